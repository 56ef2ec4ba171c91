"""Shapes and helpers shared by test_tail_reach_oracle.py (CPU) and test_gpu_tail_families.py (-m gpu): the decoder
families "tail_once" must hold on, where a tap's tail starts, and the test's own count of the column tiles a decoder
run leaves out.  Nothing the count is made of comes from the decoder under test: the reach of a launch is
restated here (`own_reach`; test_tail_reach_oracle.py holds it, and `mbv_tail_plan`, against the oracle), the route and
tile width of a launch come from `mbv_conv_plan` on that launch's descriptor, and the two stage rules (more than 256
tiles of 128 x 384 in the default mode; at most 8 column tiles a row for the packed route) are restated from DESIGN §9."""
import numpy as np
import torch

import conv_cases as cc
from mb_istft_vits_amd import _capi, models, utils as mutils
from mb_istft_vits_amd.spec import DEC_MS

RB2 = {"resblock": "2", "resblock_dilation_sizes": [[1, 3], [1, 3], [1, 3]]}
# the seven configurations of test_tail_plan.py
CONFIGS = [("ljs_mb_istft_vits", None), ("ljs_mini_mb_istft_vits", None), ("ljs_ms_istft_vits", None),
           ("uudb_ms_istft_vits_ms", None), ("ljs_istft_vits", None), ("ljs_mini_istft_vits", None),
           ("ljs_mini_mb_istft_vits", RB2)]


def ident(c):
    return c[0] + ("_rb2" if c[1] else "")


# ... minus the one with per-row conditioning (inert: test_gpu_tail_once.py)
GPU_FAMILIES = [c for c in CONFIGS if c[0] != "uudb_ms_istft_vits_ms"]

TAPS = ("dec_conv_pre", "dec_up_0", "dec_res_0", "dec_up_1", "dec_res_1", "x_post")
OUTS = ("o", "o_mb", "spec", "phase")
PRE, UP, C1, C2, POST, WAVE = range(6)                    # `kind` of a tail-plan row (decoder_table)

_HOST = {}


def host_net(name, overrides=None):
    """The model on the CPU, without weights: its cfg and `tail_plan()` (host only)."""
    key = (name, repr(overrides))
    if key not in _HOST:
        hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
        for k, v in (overrides or {}).items():
            hps.model[k] = v
        _HOST[key] = models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                           n_speakers=hps.data.n_speakers, **hps.model)
    return _HOST[key]


def n_steps(cfg):
    return len(cfg.resblock_dilation_sizes[0])


def plan_rows(net):
    """{(kind, stage, j, q): (rate, reach)} of `mbv_tail_plan`."""
    return {tuple(p[:4]): (p[4], p[5]) for p in net.tail_plan()}


def own_reach(cfg):
    """{(kind, stage, j, q): (rate, reach)} by the index rules restated here, for the GPU tests' arithmetic (the table
    under test is compared with it, and both with the oracle, by test_tail_reach_oracle.py).  Columns past rate * len - 1
    that the last valid z-frame reaches: a conv of kernel K, dilation d, 'same' padding adds d (K - 1) / 2; a
    ConvTranspose (k, stride u, padding (k - u) / 2) maps r to u r - u - (k - u) / 2 + k; a ResBlock's running-sum launch
    holds the maximum over the ResBlocks summed so far; conv_post (K 7 behind ReflectionPad1d((1, 0))) adds 3 + 1; iSTFT
    frame f covers sub-band samples [hop f - n_fft / 2, hop f + n_fft / 2); waveform sample n reads sub-band samples up
    to (n + 31) / bands."""
    rb2, nq = str(cfg.resblock) == "2", n_steps(cfg)
    out, rate, r = {(PRE, -1, 0, 0): (1, 3)}, 1, 3
    for stage, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        rate, r = rate * u, u * r - u - (k - u) // 2 + k
        out[(UP, stage, 0, 0)] = (rate, r)
        run = r
        for j, K in enumerate(cfg.resblock_kernel_sizes):
            x = r
            for q, d in enumerate(cfg.resblock_dilation_sizes[j]):
                x += d * (K - 1) // 2
                if not rb2:
                    out[(C1, stage, j, q)] = (rate, x)
                    x += (K - 1) // 2
                out[(C2, stage, j, q)] = (rate, x)
            run = max(run, x)
            out[(C2, stage, j, nq - 1)] = (rate, run)
        r = run
    r += 3 + 1
    out[(POST, 2, 0, 0)] = (rate, r)
    hop, n_fft, bands = cfg.gen_istft_hop_size, cfg.gen_istft_n_fft, cfg.subbands
    sub = hop * r - hop + n_fft // 2
    out[(WAVE, 2, 0, 0)] = (rate * hop * bands, sub if bands == 1 else bands * sub - bands + 1 + 31)
    return out


def closing_rows(net):
    """The plan row that closes each tap, and the waveform's: tap -> (rate, reach).  `dec_res_i` is closed by the last
    RESID_ACC launch of the stage (ResBlock 2, last step: kind C2 for both ResBlock types)."""
    by, last = plan_rows(net), n_steps(net.cfg) - 1
    return {"dec_conv_pre": by[(PRE, -1, 0, 0)], "dec_up_0": by[(UP, 0, 0, 0)], "dec_res_0": by[(C2, 0, 2, last)],
            "dec_up_1": by[(UP, 1, 0, 0)], "dec_res_1": by[(C2, 1, 2, last)], "x_post": by[(POST, 2, 0, 0)],
            "o": by[(WAVE, 2, 0, 0)]}


def tap_tail_starts(net, Tp):
    """tap or output -> (columns per row, rate, reach): row b's columns at and past rate * len_b + reach are its tail.
    Geometry from `tail_plan()` and cfg; an output the family does not have is left out."""
    cfg, rows = net.cfg, closing_rows(net)
    hop, n_fft, bands = cfg.gen_istft_hop_size, cfg.gen_istft_n_fft, cfg.subbands
    r = {k: (rows[k][0] * Tp, rows[k][0], rows[k][1]) for k in TAPS[:-1]}
    prate, preach = rows["x_post"]
    Fr = prate * Tp + 1
    r["x_post"] = r["spec"] = r["phase"] = (Fr, prate, preach)
    r["o"] = (rows["o"][0] * Tp, rows["o"][0], rows["o"][1])
    # frame f covers sub-band samples [hop f - n_fft / 2, hop f + n_fft / 2): the last one that frame
    # prate len - 1 + preach reaches, minus (hop prate len - 1)
    sub = hop * preach - hop + n_fft // 2
    if bands > 1 and cfg.decoder == DEC_MS:               # zero-stuffed: sub-band sample m sits at column bands * m
        r["o_mb"] = (bands * hop * prate * Tp, bands * hop * prate, bands * sub - bands + 1)
    elif bands > 1:
        r["o_mb"] = (hop * prate * Tp, hop * prate, sub)
    return r


def resblock_launches(net, B, Tp):
    """Every ResBlock launch of a decoder run on B rows of Tp frames, in launch order: (stage, kind, j, q, rate, reach,
    case), `case` a conv_cases.case of the launch (no lengths yet)."""
    cfg = net.cfg
    by = own_reach(cfg)
    rb2 = str(cfg.resblock) == "2"
    nq = n_steps(cfg)
    for stage in (0, 1):
        ch = cfg.upsample_initial_channel >> (stage + 1)
        for j, K in enumerate(cfg.resblock_kernel_sizes):
            for q in range(nq):
                for kind in ((C2,) if rb2 else (C1, C2)):
                    rate, reach = by[(kind, stage, j, q)]
                    dil = cfg.resblock_dilation_sizes[j][q] if (rb2 or kind == C1) else 1
                    epi = "STORE" if kind == C1 else ("RESID_ACC" if q == nq - 1 else "RESID")
                    acc = epi == "RESID_ACC"
                    yield stage, kind, j, q, rate, reach, cc.case(
                        "rb", None, B, ch, ch, rate * Tp, epi=epi, K=K, dil=dil, accum=acc and j > 0,
                        out_scale=cc.THIRD if acc and j == 2 else 1.0)


def donor_of(lens):
    return min(range(len(lens)), key=lambda b: (lens[b], b))          # smallest length, lowest index on ties


def pack_tiles(lens, num, reach, T, halo, bn=384):
    """Column tiles of the packed axis (layout): every row its columns [0, S_b') — S_b rounded up to 32,
    clamped to T, the donor whole — and a gap of the halo rounded up to 32, in blocks of 32 columns."""
    donor, blocks = donor_of(lens), 0
    for b, n in enumerate(lens):
        sp = T if b == donor else min(T, -(-min(T, n * num + reach) // 32) * 32)
        blocks += -(-sp // 32) + -(-halo // 32)
    return -(-blocks // (bn // 32))


def launch_left_out(c, lens, rate, reach):
    """(tiles the launch leaves out, what whole-tile maps alone would leave out, "pack" / "map" / None).  The launch
    takes a map only where its trimmed plan exists and names the route of its untrimmed one; it packs where its rows are
    at most 8 column tiles long and the planner grants the packed route to its descriptor."""
    T, B = c["T"], c["B"]
    plain = cc.plan(cc.desc(c))
    ct = dict(c, trim=(rate, reach, list(lens)))
    try:
        trimmed = cc.plan(cc.desc(ct))
    except _capi.MbvError:                                # a kernel without trimmed launches (narrow)
        return 0, 0, None
    if trimmed["route"] != plain["route"]:                # the option never changes a route: every tile is kept
        return 0, 0, None
    bn, donor = trimmed["bn"], donor_of(lens)
    full = -(-T // bn)
    by_map = sum(full - -(-min(T, rate * n + reach) // bn) for b, n in enumerate(lens) if b != donor)
    d = cc.desc(ct)
    d.tail_once = 2
    if full <= 8 and cc.plan(d)["route"] == "TAIL_PACK":
        assert bn == 384
        return max(0, B * full - pack_tiles(lens, rate, reach, T, (c["K"] - 1) * c["dil"])), by_map, "pack"
    return by_map, by_map, "map"


def decoder_left_out(net, lens, Tp, mode):
    """The column tiles one masked decoder run leaves out under `tail_once = mode`, as (total, maps alone,
    {stage: sorted routes of its launches}) in the test's own arithmetic."""
    B = len(lens)
    total = maps = 0
    how = {0: set(), 1: set()}
    for stage, kind, j, q, rate, reach, c in resblock_launches(net, B, Tp):
        stage_tiles = B * -(-c["T"] // 384) * -(-c["Cout"] // 128)
        if B < 2 or mode == 0 or (mode == 1 and stage_tiles <= 256):
            continue
        n, m, h = launch_left_out(c, lens, rate, reach)
        total, maps = total + n, maps + m
        how[stage].add(str(h))
    return total, maps, {k: sorted(v) for k, v in how.items()}


# ------------------------------------------------------------------ GPU side
_NETS = {}


def gpu_net(name, overrides=None):
    from gpu_util import make_net
    key = (name, repr(overrides))
    if key not in _NETS:
        _NETS[key] = make_net(name, overrides=overrides)[0]
    return _NETS[key]


def make_z(net, lens, Tp, seed=5):
    z = torch.randn(len(lens), net.cfg.inter_channels, Tp, generator=torch.Generator().manual_seed(seed)).cuda()
    for b, n in enumerate(lens):
        z[b, :, n:] = 0                                   # (the decoder masks at the lengths anyway: z * y_mask)
    return z


def decode(net, z, lens):
    """Every tap and every output the family has of one masked decoder run, as [B, -1] tensors; shapes from the model."""
    B, _, Tp = z.shape
    outs = net._alloc_decoder_outputs(B, Tp, z.device)
    net._decode_masked_into(z, None, lens, outs)
    r = {k: net.read_stage(k).reshape(B, -1).clone() for k in TAPS}
    r.update({k: t.reshape(B, -1) for k, t in zip(OUTS, outs) if t is not None})
    return r


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def assert_rows_alone(net, z, lens, got, rows, what):
    """Rows `rows` of a batch decode `got` are bitwise their B = 1 decode at the same T'; one row moves no counter."""
    before = net.tail_dropped()
    for b in sorted(set(rows)):
        alone = decode(net, z[b:b + 1], lens[b:b + 1])
        for k in got:
            assert torch.equal(got[k][b], alone[k][0]), (what, k, b, float((got[k][b] - alone[k][0]).abs().max()))
    assert net.tail_dropped() == before


def seeded_lens(rs, Tp, dup_min):
    """B from 2 .. 8, lengths from 0 .. T', one row pinned to T'; dup_min: the minimum again at a higher index."""
    B = int(rs.randint(2, 9))
    lens = [int(v) for v in rs.randint(0, Tp + 1, size=B)]
    whole = int(rs.randint(B))
    lens[whole] = Tp
    if dup_min:
        first = donor_of(lens)
        later = [b for b in range(first + 1, B) if b != whole]
        if later:
            lens[later[int(rs.randint(len(later)))]] = lens[first]
    return lens


def boundary_lens(net, Tp):
    """Lengths at which a reach one column short shows: for a ResBlock launch that takes a map, S_b - 1 = rate * len +
    reach - 1 is the first column of a tile, so a map built from reach - 1 drops the tile that holds the last column row b
    still reaches.  (Only launches with an odd reach have such a length: rates and tile widths are even.)  The first
    and the last such length of every launch, as vectors [T', 0, six of them at most]: the row of length 0 is the donor,
    so every one of them is a row that drops tiles."""
    found = set()
    for stage, kind, j, q, rate, reach, c in resblock_launches(net, 5, Tp):
        try:
            bn = cc.plan(cc.desc(dict(c, trim=(rate, reach, [Tp] * 5))))["bn"]
        except _capi.MbvError:
            continue
        hits = [n for n in range(1, Tp) if (rate * n + reach - 1) % bn == 0 and rate * n + reach - 1 < c["T"]]
        found |= set(hits[:1] + hits[-1:])
    found = sorted(found)
    return [[Tp, 0] + found[i:i + 6] for i in range(0, len(found), 6)]


def spread_lens(B, Tp, per, zeros):
    """The B = 128 spread of test_gpu_tail_once.py with what the builders past 256 rows need: the minimum 0 at the two
    rows `zeros` (behind row 256, in two threads' runs of `per` rows), a minimum-plus-one in front of them at row 3,
    rows 0 and B - 1 whole, short rows at 255 / 256 / 257 and on both sides of the run boundaries around each zero."""
    lens = [1 + (37 * b) % Tp for b in range(B)]
    short = {255, 256, 257}
    for zb in zeros:
        lo = zb // per * per
        short |= {lo - 1, lo, lo + per - 1, lo + per}
    for b in short:
        if 0 < b < B - 1:
            lens[b] = 2 + b % 5
    lens[0] = lens[B - 1] = Tp
    lens[3] = 1
    for zb in zeros:
        lens[zb] = 0
    assert min(zeros) > 256 and zeros[0] // per != zeros[1] // per and donor_of(lens) == min(zeros)
    return lens
