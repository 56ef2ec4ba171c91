""""tail_once", host side (no GPU): the reach table of `mbv_tail_plan` against the decoder's receptive field, and the
tail map's arithmetic (csrc/ops.hip tail_map_kernel, restated here) against the rule it must keep: a tile that holds
a column below S_b = rate * len_b + reach is never dropped.

What this file does not establish: that the reach numbers themselves are right.  `mbv_decoder_context` is the same
index rules walked backwards, and the launches between the first and the last are only checked to be non-decreasing.
test_tail_reach_oracle.py measures every tap's reach, and that of every launch inside a ResBlock, on the oracle."""
import pytest
import torch

from mb_istft_vits_amd import models, synth, utils as mutils
from oracle import ref_infer

RB2 = {"resblock": "2", "resblock_dilation_sizes": [[1, 3], [1, 3], [1, 3]]}
CONFIGS = [("ljs_mb_istft_vits", None), ("ljs_mini_mb_istft_vits", None), ("ljs_ms_istft_vits", None),
           ("uudb_ms_istft_vits_ms", None), ("ljs_istft_vits", None), ("ljs_mini_istft_vits", None),
           ("ljs_mini_mb_istft_vits", RB2)]
IDS = [c[0] + ("_rb2" if c[1] else "") for c in CONFIGS]

# y_lengths of the headline benchmark batch (ljs_mb, B = 64, T_text = 200, synthetic checkpoint 1234)
BENCH_LENS = [551, 504, 482, 479, 562, 467, 447, 502, 512, 511, 499, 479, 476, 527, 490, 504, 523, 469, 496, 498, 511,
              511, 495, 485, 501, 532, 518, 476, 443, 493, 487, 542, 482, 463, 471, 460, 566, 482, 528, 549, 516, 518,
              483, 455, 506, 521, 462, 469, 491, 491, 499, 515, 467, 489, 466, 497, 538, 525, 470, 459, 505, 497, 521,
              440]


_NETS = {}


def _net(name, overrides=None):
    key = (name, repr(overrides))
    if key not in _NETS:
        hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
        for k, v in (overrides or {}).items():
            hps.model[k] = v
        _NETS[key] = models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                           n_speakers=hps.data.n_speakers, **hps.model)
    return _NETS[key]


@pytest.mark.parametrize("name,overrides", CONFIGS, ids=IDS)
def test_reach_of_the_last_launch_is_the_decoder_context(name, overrides):
    net = _net(name, overrides)
    plan = net.tail_plan()
    kind, _, _, _, rate, reach = plan[-1]
    assert kind == 5 and rate == net.cfg.samples_per_frame
    # a sample of frame s reads z-frames [s - L, s + R]: z-frame t reaches the samples of frames [t - R, t + L], so
    # the reach to the right, in whole z-frames, is the context mbv_decoder_context calls L (25 for the multiband
    # and multistream decoders, 13 for the single-band one)
    Lc, _ = net.decoder_context()
    assert -(-reach // rate) == Lc


@pytest.mark.parametrize("name,overrides", CONFIGS, ids=IDS)
def test_reach_never_decreases_along_a_chain(name, overrides):
    net = _net(name, overrides)
    plan = net.tail_plan()
    nq = 2 if overrides else 3
    assert len(plan) == 1 + 2 * (1 + 3 * nq * (1 if overrides else 2)) + 2
    assert [p[0] for p in plan[:2]] == [0, 1] and [p[0] for p in plan[-2:]] == [4, 5]
    frames = lambda p: p[5] / p[4]                 # reach in z-frames
    first_kind = 3 if overrides else 2             # (ResBlock2 has one conv per step: kind 3 only)
    stage_in, prev = {}, plan[0]
    for p in plan[1:]:
        kind, stage, j, q = p[:4]
        if kind == 1:
            stage_in[stage] = p
        # a ResBlock starts from its stage's upsampled input, everything else from the launch before it
        src = stage_in[stage] if kind == first_kind and q == 0 else prev
        assert frames(p) >= frames(src), (src, p)
        if kind in (2, 3):
            assert p[4] == src[4] and p[5] >= src[5], (src, p)
        prev = p
    # the launch that closes a stage carries the maximum over the three ResBlocks
    for stage in (0, 1):
        ends = [p[5] for p in plan if p[1] == stage and p[0] == 3 and p[3] == nq - 1]
        assert ends == sorted(ends) and ends[-1] == max(p[5] for p in plan if p[1] == stage and p[0] in (2, 3))


def _kept_tiles(lens, num, reach, T, BN):
    """tail_map_kernel: the tiles every row keeps (a prefix of its ceil(T / BN) column tiles) and the donor."""
    full = -(-T // BN)
    donor = min(range(len(lens)), key=lambda b: (lens[b], b))
    kept = []
    for b, n in enumerate(lens):
        lim = min(max(n * num + reach, 0), T)
        kept.append(full if b == donor else -(-lim // BN))
    return kept, donor, full


def _check_map(lens, num, reach, T, BN):
    kept, donor, full = _kept_tiles(lens, num, reach, T, BN)
    assert lens[donor] == min(lens) and donor == lens.index(min(lens))
    assert kept[donor] == full
    dropped = 0
    for b, n in enumerate(lens):
        S = min(num * n + reach, T)
        assert 0 <= kept[b] <= full
        for k in range(kept[b], full):             # every dropped tile lies wholly inside [S_b, T)
            assert k * BN >= S
        if b != donor:                             # ... and every tile wholly inside it is dropped
            assert kept[b] == -(-S // BN)
        dropped += full - kept[b]
    return dropped


@pytest.mark.parametrize("BN", [128, 384])
def test_map_drops_no_tile_with_a_column_below_the_tail(BN):
    plan = _net("ljs_mb_istft_vits").tail_plan()
    launches = [(p[4], p[5]) for p in plan if p[0] in (2, 3)]
    for Tp in (96, 566):
        for num, reach in launches:
            T = num * Tp
            for lens in ([1, Tp - 1, Tp], [Tp, 1, Tp - 1, 1], [Tp - 1, Tp - 1], [1, 1, 1]):
                _check_map(lens, num, reach, T, BN)
            assert _check_map([Tp] * 5, num, reach, T, BN) == 0          # all rows at the padded length: nothing to drop


def test_map_on_the_bench_batch():
    net = _net("ljs_mb_istft_vits")
    sd = synth.make_state_dict(net.cfg, 1234)
    x, xl, _ = synth.synthetic_batch(net.cfg, 64, 200, seed=0, ragged=False)
    W = ref_infer.Weights(sd)
    with torch.no_grad():
        xe, m_t, logs_t, x_mask = ref_infer.text_encoder(W, net.cfg, torch.as_tensor(x).long(), torch.as_tensor(xl).long())
        logw = ref_infer.duration_predictor(W, net.cfg, xe, x_mask, None)
        y_lengths = ref_infer.length_regulate(logw, x_mask, m_t, logs_t, 1.0, None)[1]
    assert [int(v) for v in y_lengths.tolist()] == BENCH_LENS
    assert sum(BENCH_LENS) == 31773 and min(BENCH_LENS) == 440 and max(BENCH_LENS) == 566
    Tp = max(BENCH_LENS)
    plan = net.tail_plan()
    share = {}
    for p in plan:
        if p[0] not in (2, 3):
            continue
        num, reach = p[4], p[5]
        d = _check_map(BENCH_LENS, num, reach, num * Tp, 384)
        share.setdefault(p[1], []).append(d / (64 * -(-num * Tp // 384)))
    # the issue's table: 2 to 4 % of stage 1's tiles and 7.5 to 9 % of stage 2's lie wholly in a tail
    assert 0.005 <= min(share[0]) and max(share[0]) <= 0.05, share[0]
    assert 0.07 <= min(share[1]) and max(share[1]) <= 0.12, share[1]
