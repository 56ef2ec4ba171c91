"""The reach table of `mbv_tail_plan` against the oracle (no GPU; the built library only for the table itself).
test_tail_plan.py checks the table against its own inverse (`mbv_decoder_context`, the same index rules walked
backwards); here the numbers are MEASURED: the oracle decodes a z of one row twice, the second time with its last valid
frame changed, and the last column of every tap at which the two runs differ is how far that frame reaches.  Inside a
ResBlock the oracle has no taps, so the block is restated from its own weights with `ref_infer.conv_same`.

Measured in the oracle's fp32, seven configurations (columns past rate * len - 1):

    family          dec_conv_pre  dec_up_0  dec_res_0  dec_up_1  dec_res_1  x_post
    MB, MS, uudb               3        18         78       318        378     382
    single-band                3        28         88       708        768     772
    ResBlock2                  3        18         38       158        178     182

The waveform `o`: measured <= planned, and closer than half a z-frame (128 samples) — the outermost taps of the PQMF /
learned synthesis filter and the Hann window's zero edge fall below fp32 resolution."""
import pytest
import torch
import torch.nn.functional as F

import tail_once_cases as tc
from mb_istft_vits_amd import synth
from oracle import ref_infer

IDS = [tc.ident(c) for c in tc.CONFIGS]
TABLE = {"mb": (3, 18, 78, 318, 378, 382), "sb": (3, 28, 88, 708, 768, 772), "rb2": (3, 18, 38, 158, 178, 182)}
T_PAD, VALID = 48, 9


def _last_diff(a, b):
    """The last column at which two [1, C, T] tensors differ."""
    cols = (a != b).any(dim=1)[0].nonzero()
    assert cols.numel(), "the change did not reach this tensor"
    return int(cols.max())


@pytest.mark.parametrize("name,overrides", tc.CONFIGS, ids=IDS)
def test_reach_of_every_tap_is_what_the_oracle_shows(name, overrides):
    net = tc.host_net(name, overrides)
    cfg = net.cfg
    W = ref_infer.Weights(synth.make_state_dict(cfg, 1234))
    gen = torch.Generator().manual_seed(7)
    z = torch.randn(1, cfg.inter_channels, T_PAD, generator=gen)
    z[:, :, VALID:] = 0
    z2 = z.clone()
    z2[0, :, VALID - 1] += torch.randn(cfg.inter_channels, generator=gen)
    g = 0.3 * torch.randn(1, cfg.gin_channels, 1, generator=gen) if cfg.gin_channels else None
    runs = []
    with torch.no_grad():
        for zz in (z, z2):
            taps = {}
            taps["o"] = ref_infer.decode(W, cfg, zz, g, taps)[0]
            runs.append(taps)
    rows = tc.closing_rows(net)
    measured = {k: _last_diff(runs[0][k], runs[1][k]) - (rows[k][0] * VALID - 1) for k in tc.TAPS + ("o",)}
    planned = {k: rows[k][1] for k in measured}
    gap = planned["o"] - measured["o"]
    print("%s: reach measured %s planned %s; o planned - measured = %d samples"
          % (tc.ident((name, overrides)), [measured[k] for k in tc.TAPS], [planned[k] for k in tc.TAPS], gap))
    for k in tc.TAPS:
        assert measured[k] == planned[k], (k, measured[k], planned[k])
    family = "rb2" if overrides else ("sb" if cfg.subbands == 1 else "mb")
    assert tuple(measured[k] for k in tc.TAPS) == TABLE[family]
    assert rows["o"][0] == cfg.samples_per_frame
    assert 0 <= gap < cfg.samples_per_frame // 2, gap


@pytest.mark.parametrize("name,overrides", tc.CONFIGS, ids=IDS)
def test_the_table_is_the_rules_restated(name, overrides):
    """Every row of `mbv_tail_plan` equals `tail_once_cases.own_reach`, the arithmetic the GPU tests count tiles with."""
    net = tc.host_net(name, overrides)
    assert tc.plan_rows(net) == tc.own_reach(net.cfg)


BLOCKS = [("ljs_mini_mb_istft_vits", None), ("ljs_mb_istft_vits", None), ("ljs_mini_mb_istft_vits", tc.RB2),
          ("ljs_mb_istft_vits", tc.RB2)]
T_BLOCK, AT = 512, 200


@pytest.mark.parametrize("name,overrides", BLOCKS, ids=[tc.ident(c) for c in BLOCKS])
def test_reach_of_the_launches_inside_a_resblock(name, overrides):
    """Both stages, every ResBlock, after every conv: an input changed in column 200 alone changes the launch's output up
    to column 200 + reach(launch) - reach(ups[stage]) and no further.  A RESID_ACC launch writes the running sum, so
    the plan holds the maximum over the ResBlocks summed so far."""
    net = tc.host_net(name, overrides)
    cfg = net.cfg
    W = ref_infer.Weights(synth.make_state_dict(cfg, 1234))
    by = tc.plan_rows(net)
    rb2, nq = str(cfg.resblock) == "2", tc.n_steps(cfg)
    lrelu = lambda v: F.leaky_relu(v, ref_infer.LRELU_SLOPE)
    for stage in (0, 1):
        ch = cfg.upsample_initial_channel >> (stage + 1)
        base = by[(tc.UP, stage, 0, 0)][1]
        gen = torch.Generator().manual_seed(30 + stage)
        x0 = torch.randn(1, ch, T_BLOCK, generator=gen)
        x1 = x0.clone()
        x1[0, :, AT] += torch.randn(ch, generator=gen)
        running = 0
        for j in range(3):
            pre = "dec.resblocks.%d" % (stage * 3 + j)
            xa, xb = x0, x1
            for q, d in enumerate(cfg.resblock_dilation_sizes[j]):
                with torch.no_grad():
                    if rb2:
                        w, b = W.w(pre + ".convs.%d" % q), W.b(pre + ".convs.%d" % q)
                        xa, xb = (ref_infer.conv_same(lrelu(v), w, b, d) + v for v in (xa, xb))
                    else:
                        w, b = W.w(pre + ".convs1.%d" % q), W.b(pre + ".convs1.%d" % q)
                        ta, tb = (ref_infer.conv_same(lrelu(v), w, b, d) for v in (xa, xb))
                        assert _last_diff(ta, tb) - AT == by[(tc.C1, stage, j, q)][1] - base, (stage, j, q)
                        w, b = W.w(pre + ".convs2.%d" % q), W.b(pre + ".convs2.%d" % q)
                        xa, xb = (ref_infer.conv_same(lrelu(t), w, b, 1) + v for t, v in ((ta, xa), (tb, xb)))
                got = _last_diff(xa, xb) - AT
                if q == nq - 1:
                    running = max(running, got)
                    got = running
                assert got == by[(tc.C2, stage, j, q)][1] - base, (stage, j, q, got)
        print("%s stage %d: the ResBlocks reach %d columns past ups[%d]'s %d" % (tc.ident((name, overrides)), stage, running, stage, base))
