"""Cases, float64 references and bars of the WaveNet stacks: the four coupling layers of the flow (forward and reverse)
and the posterior encoder, importable without a GPU.  test_wn_stack_refs.py (CPU) proves the bars on the fp32 oracles
and on mutated restatements; test_gpu_wn_stack.py (-m gpu) runs every case through `align`, `infer_z_only` and
`voice_conversion` on both WN routes (the fused layer of csrc/wn_fused.hip, and the two-launch layer: EPI_GATE +
EPI_RES_SKIP + EPI_COUPLE of csrc/conv1d.hip) into the same `check_stage`.

Reference = `wn_stack`, the coupling layer, `flow_forward`, `flow_reverse` and `posterior_encoder` of
oracle/ref_infer.py restated dtype-generic: float64 is the reference, float32 "the fp32 oracle".  Weights come from
`synth.make_state_dict`, the weight-norm folded in float64 from the fp32 v and g (`Weights`).  Every stage is
referenced from the fp32 input of THAT stage (on the GPU: the GPU's own tensor), so errors do not chain and a failure
names its stage:  m_q from y;  z from (y, noise);  z_p from z;  z / z_hat from z_p.

The fp32 oracle has three variants, because the kernels compute different fp32 formulas:
  plain    the reference's order, torch's tanh / sigmoid;
  in_place the two-launch layer and run_coupling without a fold: every conv of csrc/conv1d.hip is one accumulator per
           output element fed one fused multiply-add at a time (`seq_conv`), and the epilogues that update a tensor in
           place START that accumulator from the tensor: EPI_RES_SKIP from h and the running skip, EPI_COUPLE from
           sign x1, so each of the H products is rounded at the size of x1 and not of the mean m.  That costs about
           sqrt(H) / 2 ulp of |x1| per coupling, 5 x the plain oracle's p99.9: this variant was added when the first MI355X
           run of the two-launch route missed the plain bars by that factor, and it reproduces that run's median, p99.9
           and maximum to within 2 %;
  folded   as do_finalize packs and gate_fast computes: W_in0 W_pre' and W_post W_rs[skip rows] composed in float64 and
           rounded once to fp32, the bias of `pre` through the mask channel of x0' = [x0 ; mask], the coupling mean
           accumulated layer by layer, and the gate (1 - 2 / (1 + 2^(2 x log2 e))) / (1 + 2^(-y log2 e)).  `fold` of a
           case says what do_finalize folds for its sizes ("pre+post", "post", "none": wn_prefold_fits /
           wn_postfold_fits of csrc/wn_fused.hip); the posterior encoder has nothing to fold, only the gate differs.

Bars, per case and stage over the valid frames t < len[b]: the median, the 99.9th percentile and the maximum of
|got - ref64| are each at most MARGIN x the fp32 oracle's own, plus one fp32 ulp of the reference's RMS.  MARGIN = 4 as
in small_op_cases.py: operation order, FMA contraction and the transcendentals cost a few ulp each, not more.  The
oracle's value is the largest over the variants of the route (`variants`): plain and folded on the fused route (and
in_place where neither fold fits, so that `post` is the EPI_COUPLE conv), plain and in_place on the two-launch route.
Frames at and beyond len[b] must be exactly 0, every output finite, and two calls must agree bit for bit.

MUTANTS (`mut=`) are deliberate mistakes that the bars must catch in every case that lists them (a case lists a mutant
only where it can show: the cond_* ones need gin_channels, the mask / halo ones a row shorter than T).

Per route and stage, the case that uses the largest share of a bar: the oracle's errors (the largest over the
route's variants), the bars from them, and the MI355X measurement (profiles/wn_stack_bars.json has every case), each
as median / p99.9 / max of |x - ref64| over the valid frames; last column: the largest share of a bar used.

    route      stage           case         oracle                           bar                              MI355X                           share
    fused      align m_q       h192_i192_g  7.64e-07 / 4.02e-06 / 6.43e-06   3.18e-06 / 1.62e-05 / 2.58e-05   2.00e-06 / 1.05e-05 / 1.43e-05   0.65
    fused      align z         h192_i192_g  7.80e-07 / 4.22e-06 / 6.40e-06   3.24e-06 / 1.70e-05 / 2.57e-05   2.04e-06 / 1.08e-05 / 1.45e-05   0.63
    fused      align z_p       h192_i192_g  2.59e-07 / 1.37e-06 / 1.75e-06   1.27e-06 / 5.70e-06 / 7.24e-06   4.12e-07 / 2.21e-06 / 3.30e-06   0.46
    fused      infer_z_only z  h160_i64_g   1.81e-07 / 9.04e-07 / 1.01e-06   8.43e-07 / 3.73e-06 / 4.15e-06   3.02e-07 / 1.70e-06 / 1.94e-06   0.47
    fused      vc z            h192_i192_g  7.80e-07 / 4.22e-06 / 6.40e-06   3.24e-06 / 1.70e-05 / 2.57e-05   2.04e-06 / 1.08e-05 / 1.45e-05   0.63
    fused      vc z_p          h192_i192_g  2.59e-07 / 1.37e-06 / 1.75e-06   1.27e-06 / 5.70e-06 / 7.24e-06   4.12e-07 / 2.21e-06 / 3.30e-06   0.46
    fused      vc z_hat        h192_i192_g  2.59e-07 / 1.33e-06 / 1.73e-06   1.15e-06 / 5.45e-06 / 7.04e-06   4.21e-07 / 2.24e-06 / 2.73e-06   0.41
    two_launch align m_q       h192_i192_g  2.06e-06 / 1.05e-05 / 1.28e-05   8.35e-06 / 4.21e-05 / 5.15e-05   1.98e-06 / 1.02e-05 / 1.60e-05   0.31
    two_launch align z         h192_i192_g  2.09e-06 / 1.11e-05 / 1.50e-05   8.47e-06 / 4.45e-05 / 6.03e-05   2.04e-06 / 1.07e-05 / 1.59e-05   0.26
    two_launch align z_p       h224_g       7.51e-07 / 6.56e-06 / 8.47e-06   3.12e-06 / 2.64e-05 / 3.40e-05   7.46e-07 / 7.16e-06 / 1.09e-05   0.32
    two_launch infer_z_only z  h192_i192_g  5.56e-07 / 4.12e-06 / 7.25e-06   2.34e-06 / 1.66e-05 / 2.91e-05   5.46e-07 / 4.23e-06 / 7.27e-06   0.25

The plain and folded oracles alone, worst case of each stage on the CPU (test_wn_stack_refs.py prints all of them):
posterior encoder 8.0e-07 / 4.3e-06 / 7.4e-06, forward flow 2.6e-07 / 1.3e-06 / 1.9e-06, reverse flow 2.6e-07 / 1.4e-06 /
1.8e-06; the folded oracle's three errors are 0.68 .. 1.2 x the plain one's in every case and stage, so the rounding of
do_finalize's folds and of gate_fast fits the margin with room.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_infer as R

MARGIN = 4.0
F64, F32 = torch.float64, torch.float32
FLOW_LAYERS, N_FLOWS, ENC_Q_LAYERS = R.FLOW_LAYERS, R.N_FLOWS, 16

MUTANTS = ("no_flip", "flip_after_reverse", "couple_sign", "cond_layer_shift", "cond_missing", "last_layer_split",
           "h_unmasked", "pre_bias_unmasked", "post_bias_once_per_layer", "skip_not_reset", "halo_from_neighbour")
_ALWAYS = ("no_flip", "flip_after_reverse", "couple_sign", "last_layer_split", "post_bias_once_per_layer", "skip_not_reset")
_COND = ("cond_layer_shift", "cond_missing")
_RAGGED = ("h_unmasked", "pre_bias_unmasked", "halo_from_neighbour")

# what is not under test is shrunk (decoder, text encoder)
SHRINK = {"upsample_initial_channel": 128, "n_layers": 1, "filter_channels": 64}


def _case(name, H, I, gin, T, lens, fold, reaches, route="fused", vc=False, mutants=None):
    assert max(lens) == T and any(l < T for l in lens)
    return dict(name=name, H=H, I=I, gin=gin, B=len(lens), T=T, lens=list(lens), fold=fold, route=route, vc=vc,
                cfg="uudb_ms_istft_vits_ms" if gin else "ljs_mini_mb_istft_vits",
                overrides=dict(SHRINK, hidden_channels=H, inter_channels=I, **({"gin_channels": gin} if gin else {})),
                mutants=tuple(mutants) if mutants is not None else _ALWAYS + (_COND if gin else ()) + _RAGGED,
                reaches=reaches)


CASES = [
    _case("h192_i192_g", 192, 192, 256, 70, [70, 1, 33, 17], "pre+post", vc=True,
          reaches="NRT = 3, Gi = 13, speaker conditioning, 11 half-units: tiles that pair two utterances and a last "
                  "tile with an empty second half"),
    _case("h96_i192", 96, 192, 0, 48, [48, 48, 31], "pre+post", reaches="NRT = 2, no conditioning, an even tile count"),
    _case("h160_i64_g", 160, 64, 64, 50, [50, 15, 32], "pre+post",
          reaches="10 gate row tiles over 4 waves (3, 3, 2, 2), Gi = 5, last layer Mr = 32: idle tile slots"),
    _case("h64_i256_g", 64, 256, 64, 50, [50, 16, 31], "post",
          reaches="Gi = 17 > 16: `pre` is not folded (wn_prefold_fits), `post` is, and skip holds I / 2 = 128 > H rows"),
    _case("h128_i128", 128, 128, 0, 33, [33, 17], "pre+post", reaches="NRT = 2 with all 8 row tiles, Gi = 9"),
    _case("h128_i384", 128, 384, 0, 33, [33, 16], "none",
          reaches="H + I / 2 = 320 > 256 rows: neither fold (wn_postfold_fits), the fused layers between pre and EPI_COUPLE"),
    _case("many_tiles", 64, 64, 0, 4000, [4000, 4000, 3990, 4000, 4000], "pre+post",
          reaches="1250 half-units = 625 tiles > the 512 workgroups of a launch: the u += gridDim.x walk",
          mutants=("no_flip", "h_unmasked", "halo_from_neighbour", "skip_not_reset")),
    _case("h224_g", 224, 192, 64, 40, [40, 15], "none", route="two_launch",
          reaches="wn_fused_supported false: the two-launch layer as the default route"),
]
BY_NAME = {c["name"]: c for c in CASES}
# the cases that run again with set_option("wn_fused", 0)
TWO_LAUNCH_AGAIN = ("h192_i192_g", "h96_i192", "h64_i256_g")
# half-units of 16 frames: a ragged case holds lengths at the edges of a half-unit and of a 32-column tile
EDGE_LENGTHS = {1, 15, 16, 17, 31, 32, 33}


def variants(c, route):
    """the fp32 oracle variants whose largest error makes the bars of a case on a route"""
    if route == "two_launch":
        return ("plain", "in_place")
    return ("plain", "folded") + (("in_place",) if c["fold"] == "none" else ())


def half_units(lens):
    return sum((l + 15) // 16 for l in lens)


# ---------------------------------------------------------------------------------------------- weights
class Weights:
    """name -> tensor of the asked dtype; weight-norm pairs are folded in float64 from the fp32 v and g, once."""

    def __init__(self, sd):
        self.sd = {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}
        self._w64 = {}

    def w(self, prefix, dtype):
        if prefix not in self._w64:
            if prefix + ".weight" in self.sd:
                self._w64[prefix] = self.sd[prefix + ".weight"].to(F64)
            else:
                self._w64[prefix] = R.fold_weight_norm(self.sd[prefix + ".weight_v"].to(F64), self.sd[prefix + ".weight_g"].to(F64))
        return self._w64[prefix].to(dtype)

    def b(self, prefix, dtype):
        return self.sd[prefix + ".bias"].to(dtype)

    def g(self, sid, dtype):
        """[B, gin, 1] speaker vectors (an exact gather), or None"""
        return None if sid is None else self.sd["emb_g.weight"][torch.as_tensor(sid).long()].to(dtype).unsqueeze(-1)


def fmask(lens, T, dtype):
    return (torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]).to(dtype).unsqueeze(1)        # [B, 1, T]


# ---------------------------------------------------------------------------------------------- the operations
def gate_plain(x, y):
    return torch.tanh(x) * torch.sigmoid(y)                      # commons.py:100-107


def gate_fast(x, y):
    """gate_fast of csrc/wn_fused.hip, in the arithmetic of x's dtype"""
    e2x = torch.exp2(x * 2.88539008177792681)
    emy = torch.exp2(y * -1.44269504088896341)
    th = 1.0 - 2.0 * (1.0 / (1.0 + e2x))
    return th * (1.0 / (1.0 + emy))


def _neighbour_halo(h, lens):
    """frames len .. len + 1 of a row taken from the next row's first frames (a wrong pairing of half-units)"""
    B, _, T = h.shape
    o = h.clone()
    for b, l in enumerate(lens):
        n = min(2, T - l)
        if n > 0:
            o[b, :, l:l + n] = h[(b + 1) % B, :, :n]
    return o


def wn_stack(W, prefix, H, h, mask, g, n_layers, lens, mut=None, gate=gate_plain, out0=None):
    """modules.py:148-176 (ref_infer.wn_stack) -> the masked sum of the skips"""
    dt = h.dtype
    out = torch.zeros_like(h) if out0 is None else out0
    gc = None
    if g is not None and mut != "cond_missing":
        gc = F.conv1d(g, W.w(prefix + ".cond_layer", dt), W.b(prefix + ".cond_layer", dt))
    for l in range(n_layers):
        q = prefix + ".in_layers.%d" % l
        a = R.conv_same(_neighbour_halo(h, lens) if mut == "halo_from_neighbour" else h, W.w(q, dt), W.b(q, dt))
        if gc is not None:
            k = (l + 1) % n_layers if mut == "cond_layer_shift" else l
            a = a + gc[:, 2 * H * k:2 * H * (k + 1)]
        acts = gate(a[:, :H], a[:, H:])
        q = prefix + ".res_skip_layers.%d" % l
        rs = F.conv1d(acts, W.w(q, dt), W.b(q, dt))
        if l < n_layers - 1:
            h = h + rs[:, :H]
            if mut != "h_unmasked":
                h = h * mask
            out = out + rs[:, H:]
        elif mut != "last_layer_split":                          # (the mutant: rows below the split go to the residual)
            out = out + rs
    return out * mask


def coupling(W, f, cfg, x0, x1, mask, g, sign, lens, mut=None, gate=gate_plain, carry=None):
    """modules.py:334-353, mean_only: forward m + x1 mask, reverse (x1 - m) mask -> (x1', the stack's skip sum)"""
    dt = x0.dtype
    p = "flow.flows.%d" % (2 * f)
    h = F.conv1d(x0, W.w(p + ".pre", dt), W.b(p + ".pre", dt))
    if mut != "pre_bias_unmasked":
        h = h * mask
    out = wn_stack(W, p + ".enc", cfg.hidden_channels, h, mask, g, FLOW_LAYERS, lens, mut, gate,
                   carry if mut == "skip_not_reset" else None)
    m = F.conv1d(out, W.w(p + ".post", dt), W.b(p + ".post", dt))
    if mut == "post_bias_once_per_layer":
        m = m + (FLOW_LAYERS - 1) * W.b(p + ".post", dt)[None, :, None]
    return x1 * mask + sign * (m * mask), out


def coupling_folded(W, f, cfg, x0, x1, mask, g, sign, fold):
    """The coupling layer as do_finalize folds it for the fused WN layers (fp32): fold = "pre+post" or "post"."""
    dt = x0.dtype
    H = cfg.hidden_channels
    p = "flow.flows.%d" % (2 * f)
    wpre = torch.cat([W.w(p + ".pre", dt)[:, :, 0], W.b(p + ".pre", dt)[:, None]], 1)        # W_pre' = [W_pre | b_pre]
    wpost = W.w(p + ".post", dt)[:, :, 0].to(F64)
    bpost = W.b(p + ".post", dt).to(F64)
    gc = None
    if g is not None:
        gc = F.conv1d(g, W.w(p + ".enc.cond_layer", dt), W.b(p + ".enc.cond_layer", dt))
    x0m = torch.cat([x0 * mask, mask], 1)                                                      # x0' = [x0 ; mask]
    h = F.conv1d(x0m, wpre[:, :, None]) if fold == "pre+post" else F.conv1d(x0, W.w(p + ".pre", dt), W.b(p + ".pre", dt)) * mask
    m = None
    for l in range(FLOW_LAYERS):
        q = p + ".enc.in_layers.%d" % l
        if l == 0 and fold == "pre+post":
            wc = torch.einsum("rkt,kc->rct", W.w(q, dt).to(F64), wpre.to(F64)).to(dt)          # W_in0[tap] W_pre'
            a = F.conv1d(x0m, wc, W.b(q, dt), padding=2)
        else:
            a = R.conv_same(h, W.w(q, dt), W.b(q, dt))
        if gc is not None:
            a = a + gc[:, 2 * H * l:2 * H * (l + 1)]
        acts = gate_fast(a[:, :H], a[:, H:])
        q = p + ".enc.res_skip_layers.%d" % l
        wrs, brs = W.w(q, dt)[:, :, 0], W.b(q, dt)
        last = l == FLOW_LAYERS - 1
        if not last:
            h = (h + F.conv1d(acts, wrs[:H, :, None], brs[:H])) * mask
        s0 = 0 if last else H
        wm = (wpost @ wrs[s0:].to(F64)).to(dt)                                                 # W_post W_rs[skip rows]
        bm = (wpost @ brs[s0:].to(F64) + (bpost if last else 0.0)).to(dt)
        part = F.conv1d(acts, wm[:, :, None], bm)
        m = part if m is None else m + part
    return x1 * mask + sign * (m * mask)


def seq_conv(x, w, acc0=None):
    """A conv as csrc/conv1d.hip sums it in fp32: one accumulator per output element, started from `acc0` (what the
    epilogue updates in place; default 0) and fed one fused multiply-add at a time, input channels in chunks of 16,
    inside a chunk tap by tap.  (The product of two fp32 is exact in float64, so the float64 sum rounded to fp32 is the
    fused multiply-add.)  The bias is the caller's: the kernel adds it behind the loop."""
    B, Cin, T = x.shape
    M, _, K = w.shape
    xp = F.pad(x, ((K - 1) // 2, (K - 1) // 2)).to(F64)
    xs = [xp[:, :, tap:tap + T].permute(1, 0, 2).reshape(Cin, 1, B * T).contiguous() for tap in range(K)]
    wk = w.to(F64).permute(1, 2, 0).reshape(Cin, K, M, 1).contiguous()
    acc32 = torch.zeros(M, B * T, dtype=F32) if acc0 is None else acc0.to(F32).permute(1, 0, 2).reshape(M, B * T).contiguous()
    acc64, tmp = acc32.to(F64), torch.empty(M, B * T, dtype=F64)
    live = [ci for ci in range(Cin) if bool(xp[:, ci].any())]    # (a channel of zeros changes nothing)
    for c0 in range(0, Cin, 16):
        for tap in range(K):
            for ci in (i for i in live if c0 <= i < c0 + 16):
                torch.addcmul(acc64, wk[ci, tap], xs[tap][ci], out=tmp)
                acc32.copy_(tmp)                                 # the one rounding of the step
                acc64.copy_(acc32)
    return acc32.reshape(M, B, T).permute(1, 0, 2).contiguous()


def _wn_in_place(W, prefix, H, h, mask, g, n_layers):
    """run_wn's two-launch layers: gate conv (EPI_GATE: bias + conditioning behind the sum, libm tanh and 1 / (1 + exp(-v)))
    and res/skip conv (EPI_RES_SKIP: the accumulators start from h and from the running skip) -> skip, unmasked"""
    gc = None
    if g is not None:
        gc = F.conv1d(g, W.w(prefix + ".cond_layer", F32), W.b(prefix + ".cond_layer", F32))
    skip = None
    for l in range(n_layers):
        q = prefix + ".in_layers.%d" % l
        rowc = W.b(q, F32)[None, :, None]
        if gc is not None:
            rowc = rowc + gc[:, 2 * H * l:2 * H * (l + 1)]
        a = seq_conv(h, W.w(q, F32)) + rowc
        acts = torch.tanh(a[:, :H]) * (1.0 / (1.0 + torch.exp(-a[:, H:])))
        q = prefix + ".res_skip_layers.%d" % l
        last = l == n_layers - 1
        s0 = skip if skip is not None else torch.zeros_like(h)
        v = seq_conv(acts, W.w(q, F32), s0 if last else torch.cat([h, s0], 1)) + W.b(q, F32)[None, :, None]
        if last:
            skip = v
        else:
            h, skip = v[:, :H] * mask, v[:, H:]
    return skip


def coupling_in_place(W, f, cfg, x0, x1, mask, g, sign):
    """run_coupling without a fold (fp32): `pre` (bias behind the sum, masked), the two-launch WN layers, and `post` with
    EPI_COUPLE, whose accumulators start from sign x1: x1' = mask sign ((sign x1 + W_post skip) + b_post)"""
    p = "flow.flows.%d" % (2 * f)
    h = (seq_conv(x0, W.w(p + ".pre", F32)) + W.b(p + ".pre", F32)[None, :, None]) * mask
    skip = _wn_in_place(W, p + ".enc", cfg.hidden_channels, h, mask, g, FLOW_LAYERS)
    acc = seq_conv(skip * mask, W.w(p + ".post", F32), sign * x1)
    return sign * (acc + W.b(p + ".post", F32)[None, :, None]) * mask


def _couple(W, f, cfg, x, mask, g, sign, lens, mut, variant, fold, carry):
    half = cfg.inter_channels // 2
    x0, x1 = x[:, :half], x[:, half:]
    if variant == "in_place":
        return torch.cat([x0, coupling_in_place(W, f, cfg, x0, x1, mask, g, sign)], 1), None
    if variant == "folded" and fold != "none":
        return torch.cat([x0, coupling_folded(W, f, cfg, x0, x1, mask, g, sign, fold)], 1), None
    y1, out = coupling(W, f, cfg, x0, x1, mask, g, sign, lens, mut, gate_fast if variant == "folded" else gate_plain, carry)
    return torch.cat([x0, y1], 1), out


def flow_forward(W, cfg, z, lens, g, dtype, mut=None, variant="plain", fold="pre+post"):
    """models.py:209-210: coupling layer, then Flip, flows 0 .. 3"""
    x, mask, carry = z.to(dtype), fmask(lens, z.shape[2], dtype), None
    g = None if g is None else g.to(dtype)
    for f in range(N_FLOWS):
        x, carry = _couple(W, f, cfg, x, mask, g, 1.0, lens, mut, variant, fold, carry)
        if mut != "no_flip":
            x = torch.flip(x, [1])
    return x


def flow_reverse(W, cfg, z_p, lens, g, dtype, mut=None, variant="plain", fold="pre+post"):
    """models.py:212-214: Flip, then the coupling layer, flows 3 .. 0"""
    x, mask, carry = z_p.to(dtype), fmask(lens, z_p.shape[2], dtype), None
    g = None if g is None else g.to(dtype)
    for f in reversed(range(N_FLOWS)):
        if mut not in ("no_flip", "flip_after_reverse"):
            x = torch.flip(x, [1])
        x, carry = _couple(W, f, cfg, x, mask, g, 1.0 if mut == "couple_sign" else -1.0, lens, mut, variant, fold, carry)
        if mut == "flip_after_reverse":
            x = torch.flip(x, [1])
    return x


def posterior_encoder(W, cfg, y, lens, g, noise, dtype, mut=None, variant="plain"):
    """models.py:239-246 -> (z, m_q), both masked; `noise` replaces torch.randn_like(m)"""
    y, mask = y.to(dtype), fmask(lens, y.shape[2], dtype)
    g = None if g is None else g.to(dtype)
    if variant == "in_place":
        h = (seq_conv(y, W.w("enc_q.pre", F32)) + W.b("enc_q.pre", F32)[None, :, None]) * mask
        out = _wn_in_place(W, "enc_q.enc", cfg.hidden_channels, h, mask, g, ENC_Q_LAYERS) * mask
        stats = (seq_conv(out, W.w("enc_q.proj", F32)) + W.b("enc_q.proj", F32)[None, :, None]) * mask
        m, logs = stats[:, :cfg.inter_channels], stats[:, cfg.inter_channels:]
        return (m + noise.to(F32) * torch.exp(logs)) * mask, m
    h = F.conv1d(y, W.w("enc_q.pre", dtype), W.b("enc_q.pre", dtype))
    if mut != "pre_bias_unmasked":
        h = h * mask
    out = wn_stack(W, "enc_q.enc", cfg.hidden_channels, h, mask, g, ENC_Q_LAYERS, lens, mut,
                   gate_fast if variant == "folded" else gate_plain)
    stats = F.conv1d(out, W.w("enc_q.proj", dtype), W.b("enc_q.proj", dtype)) * mask
    m, logs = stats[:, :cfg.inter_channels], stats[:, cfg.inter_channels:]
    return (m + noise.to(dtype) * torch.exp(logs)) * mask, m


# which stages a mutant can show in
SHOWS_IN = {"enc": _COND + ("last_layer_split",) + _RAGGED,
            "fwd": tuple(m for m in MUTANTS if m not in ("flip_after_reverse", "couple_sign")),
            "rev": MUTANTS}


# ---------------------------------------------------------------------------------------------- inputs
def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def inputs(c, n_vocab=59, spec_channels=513):
    """Everything a case feeds the entry points, deterministic: the recording y = |randn| 3 (as the goldens' generator
    draws it), the posterior's noise, a text shorter than the recording with durations whose row sums are the lengths,
    speakers (src != tgt where a case converts)."""
    g = gen(c["name"])
    B, T, lens = c["B"], c["T"], c["lens"]
    t_text = 4
    x_lengths = [min(t_text, l) for l in lens]
    x = torch.randint(1, n_vocab, (B, t_text), generator=g)
    dur = torch.zeros(B, t_text, dtype=torch.int64)
    for b, (l, n) in enumerate(zip(lens, x_lengths)):
        x[b, n:] = 0
        dur[b, :n] = l // n
        dur[b, 0] += l - (l // n) * n
    assert dur.sum(1).tolist() == lens
    out = dict(x=x, x_lengths=torch.tensor(x_lengths), durations=dur, y_lengths=torch.tensor(lens),
               y=torch.randn(B, spec_channels, T, generator=g).abs() * 3, noise=torch.randn(B, c["I"], T, generator=g),
               prior_noise=torch.randn(B, c["I"], T, generator=g), sid=None, sid_tgt=None)
    if c["gin"]:
        out["sid"] = torch.tensor([(3 + 5 * b) % 12 for b in range(B)])
        out["sid_tgt"] = torch.tensor([(4 + 7 * b) % 12 for b in range(B)])
        assert not bool((out["sid"] == out["sid_tgt"]).any())
    return out


# ---------------------------------------------------------------------------------------------- the bars
def ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if x > 0 else 0.0


def _valid(lens, T):
    return torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]                           # [B, T]


def err_stats(a, ref, lens):
    """(median, p99.9, max) of |a - ref| over the valid frames"""
    v = _valid(lens, ref.shape[2])[:, None, :].expand_as(ref)
    e = (a.to(F64) - ref)[v].abs()
    e = torch.nan_to_num(e, nan=float("inf"))
    s = torch.sort(e)[0]
    n = s.numel()
    return float(s[(n - 1) // 2]), float(s[min(n - 1, int(np.ceil(0.999 * (n - 1))))]), float(s[-1])


def bars(ref, oracles, lens):
    """-> ((median, p99.9, max) bars, the oracle's own three: the largest over the variants given, ulp of the RMS)"""
    v = _valid(lens, ref.shape[2])[:, None, :].expand_as(ref)
    ulp = ulp32(float(ref[v].pow(2).mean().sqrt()))
    o = [max(s) for s in zip(*(err_stats(x, ref, lens) for x in oracles))]
    return tuple(MARGIN * x + ulp for x in o), tuple(o), ulp


STAT_NAMES = ("median", "p99.9", "max")


def check_stage(what, got, ref, oracles, lens, report=None):
    """got: fp32 [B, C, T] of the code under test; ref: float64; oracles: the fp32 oracle variants of this route."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(ref).all()), (what, "reference not finite")
    assert bool(torch.isfinite(got).all()), (what, "non-finite output", int((~torch.isfinite(got)).sum()))
    pad = ~_valid(lens, ref.shape[2])[:, None, :].expand_as(ref)
    assert bool((got[pad] == 0).all()), (what, "frames at and beyond len[b] must be exactly 0", int((got[pad] != 0).sum()))
    bar, orc, ulp = bars(ref, oracles, lens)
    e = err_stats(got, ref, lens)
    print("%-34s " % what + "  ".join("%s %.3g (oracle %.3g, bar %.3g)" % (n, x, o, b) for n, x, o, b in zip(STAT_NAMES, e, orc, bar))
          + "  ulp(rms) %.3g" % ulp)
    if report is not None:
        report[what] = {"got": list(e), "oracle": list(orc), "bar": list(bar), "share": [x / b for x, b in zip(e, bar)]}
    for n, x, b in zip(STAT_NAMES, e, bar):
        assert x <= b, (what, n, x, "bar", b, "oracle", orc, "ulp", ulp)
