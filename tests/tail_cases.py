"""Cases, float64 reference and bars of the one-shot waveform tails `istft_pqmf_kernel` and `istft_single_kernel`
(csrc/istft_pqmf.hip, csrc/istft_tail.inc), importable without a GPU.  test_tail_refs.py (CPU) proves the bars on the
fp32 oracles and on the mutants; test_gpu_tail.py (-m gpu) runs every case through the entry points into `tail_check`.
The streaming, ragged and pooled tails are pinned bitwise to the one-shot launch by their own tests.

Reference = `tail_compute(case, inp, float64)`: spec, phase, the sub-band signal (`omb`: y_mb, or the zero-stuffed,
x4 `up` of the multi-stream layout) and `o`, in float64 FROM THE fp32 INPUTS OF THE VARIANT:
    plain   x_post: exp(x), pi sin(x)
    pre     the already rounded prescaled fp32 rows xm = x log2(e), xp = x / (2 pi): 2^xm, pi sin(2 pi xp)
    polar   the fp32 (spec, phase) themselves
with the inverse-DFT basis and the periodic Hann window exact, and the synthesis bank the fp32
`pqmf_synthesis_filter` / the trainable [4, 63] taps taken to float64.  (The kernel's factorised PQMF_G * PQMF_C taps
differ from that bank by their own rounding: that is in the bound, not in the reference.)

fp32 oracles (`style`): `plain`, the reference's formula in fp32 torch (ref_infer's fp32 basis and window);
`turns`, the same written as the hardware-transcendental path writes it: exp2(x log2e), the sine of an argument
rounded in turns, 0.5 s fed to cos / sin, the functions themselves correctly rounded.  The exact-math route is held to
`plain`, the hardware route to the larger of the two.

Bars, per element: |y - y64| <= TOL[k] u A + FLOOR (small_op_cases.py), A from `tail_bound`: first-order propagation
of one rounding per operation through the formula as the kernel writes it -- |x| |d/dx| for the scalings of the
pre-activations (x log2e, x / 2 pi, pi s, and their constants), DEPTH roundings along a path of the packed 16-point
inverse transform and the window, the overlap-add, the reciprocal envelope, and for `o` the 63-tap sum with NK
roundings per term (the taps' own rounding, the modulation rows, the fma chain).  Per case: median and 99.9th
percentile at most MARGIN = 4 x the oracle's, plus one fp32 ulp of the reference's RMS.  FLOOR covers the planted
log-magnitude of -100, which is flushed.

TOL[k] = 4 x the worst err / (u A) of the fp32 oracles over the committed cases and variants, rounded up to one digit
(test_tail_refs.py measures and asserts it):

    output       oracle worst err / (u A)          TOL   MI355X exact route   hardware route   (profiles/tail_bars.json)
    tail_spec    0.996  (plain, x ln 2 of `pre`)     4     1.22  (0.30 of TOL)  1.22  (0.30)     quantile bars used: 0.27 / 0.27
    tail_phase   0.822  (turns, x / 2 pi rounded)    4     0.754 (0.19)         2.86  (0.71)     0.25 / 0.25
    tail_omb     0.577  (turns)                      3     0.561 (0.19)         0.578 (0.19)     0.28 / 0.32
    tail_o       0.603  (turns, single band)         3     0.455 (0.15)         0.597 (0.20)     0.44 / 0.33
The figures beyond the oracles' own: the spec ratio 1.22 (the device's exp; both routes, to every digit) and the
hardware route's phase ratio 2.86 (the turns argument x / (2 pi) rounded to fp32, then v_sin_f32 on it).

The multi-band kernel missed the 99.9 % bar of `omb` on mb_tp1_s07 when these tests were first run (1.0e-6 against
1.7e-7, every route): the entries 7 and 9 of its edge table of squared window values (WSQ16) were 0.92533011 for
0.92532811, which scaled the first and last two odd samples of every utterance by 1 - 1.4e-6.  The table was
corrected; the mutant `wsq_7_9` is that mistake.

Entry points and the template instantiations they reach (istft_pqmf_kernel<TM, NT, FIXED, FAST, PRE, POLAR>,
istft_single_kernel<FAST, PRE, POLAR>):
    mbv_istft_pqmf        filter NULL / given -> FIXED 1 / 0; option istft_exact 0 / 1 -> FAST 1 / 0; multistream bit 1
                          -> PRE; bit 0: the o_mb layout; POLAR 0
    mbv_istft_finalize    multi-band net -> <FIXED 1, FAST, PRE 0, POLAR 1>; multi-stream net -> <FIXED 0, ...>;
                          single-band net -> istft_single_kernel<FAST, 0, POLAR 1>
    mbv_op_istft_single   istft_single_kernel<FAST, PRE, POLAR 0>

Mutants (MUTANTS): every one fails at least one committed (case, variant).  `dc_imag` / `nyq_imag`: in the matrix form
of the inverse transform the imaginary parts of bins 0 and 8 multiply sin(0) and sin(pi n) and cannot matter; in the
packed form the kernel uses (Z_0 = A_0 + j D_0) they can, and the mutants are that mistake: Im X_0 / Im X_8 kept in Z_0.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import small_op_cases as sc
from oracle import ref_infer as R
from small_op_cases import F32, F64, FLOOR, MARGIN, U, gen, ulp32

TOL = {"tail_spec": 4.0, "tail_phase": 4.0, "tail_omb": 3.0, "tail_o": 3.0}
sc.TOL.update(TOL)                      # (small_op_cases.Stats looks its kernels up there)
Stats = sc.Stats
DEPTH = 12.0                            # roundings along a path of irfft16_hann (A / D, twiddle, Z, two radix stages, T, sum, window)
NK = {"fixed": 26.0, "trainable": 66.0}  # per term of the synthesis sum: taps, modulation rows, the fma chain
N_FFT, HOP, NB = 16, 4, 9
LOG2E, INV2PI = 1.44269504088896341, 0.15915494309189535

STYLES = ("plain", "turns")          # the fp32 oracles of the bars (`packed`: see test_tail_refs.py)
MUTANTS = ["hann_sym", "env_flat", "env_last_frame", "nyq_imag", "dc_imag", "tap0", "tap62", "no_gain4", "pad_30_32",
           "band_swap", "phase_no_pi", "prescale_ignored", "stuff_phase", "halo_zero", "trainable_reversed", "wsq_7_9"]


def tail_case(name, kind, n, std):
    """kind 'mb': n = Tp z-frames (F = 16 n + 1, tile 480 sub-band samples = 7.5 z-frames); 'sb': n = F - 1 quads
    (tile 252)."""
    return dict(name=name, kind=kind, n=n, std=std, B=3, K=4 if kind == "mb" else 1, F=(16 * n + 1) if kind == "mb" else n + 1)


TAIL_CASES = [
    tail_case("mb_tp1_s07", "mb", 1, 0.7), tail_case("mb_tp7_s2", "mb", 7, 2.0), tail_case("mb_tp8_s07", "mb", 8, 0.7),
    tail_case("mb_tp15_s2", "mb", 15, 2.0), tail_case("mb_tp16_s07", "mb", 16, 0.7), tail_case("mb_tp16_s2", "mb", 16, 2.0),
    tail_case("sb_q1_s07", "sb", 1, 0.7), tail_case("sb_q3_s2", "sb", 3, 2.0), tail_case("sb_q251_s07", "sb", 251, 0.7),
    tail_case("sb_q252_s2", "sb", 252, 2.0), tail_case("sb_q253_s07", "sb", 253, 0.7), tail_case("sb_q505_s2", "sb", 505, 2.0),
]
# (variant, bank, layout) a case is run in; layout: the o_mb of the multi-band ('mb') or of the multi-stream decoder ('ms')
MB_VARIANTS = [("plain", "fixed", "mb"), ("pre", "fixed", "ms"), ("polar", "fixed", "mb"), ("plain", "trainable", "ms"),
               ("pre", "trainable", "mb"), ("polar", "trainable", "ms")]
SB_VARIANTS = [("plain", None, None), ("pre", None, None), ("polar", None, None)]


def with_variant(c, variant, bank=None, layout=None):
    return dict(c, variant=variant, bank=bank, layout=layout, name="%s/%s%s%s" % (
        c["name"], variant, "/" + bank if bank else "", "/" + layout if layout else ""))


def runs():
    return [with_variant(c, *v) for c in TAIL_CASES for v in (MB_VARIANTS if c["kind"] == "mb" else SB_VARIANTS)]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = next(x for x in TAIL_CASES if x["name"] == name)
    g = gen(name)
    B, K, Fr = c["B"], c["K"], c["F"]
    x = torch.randn(B, K, 2 * NB, Fr, generator=g)
    x[:, :, :NB] *= c["std"]
    x[:, :, NB + 5] *= 64.0 / float(x[:, :, NB + 5].abs().max())          # one phase bin per band: |x| reaches 64
    x[0, 0, 3, Fr // 2] = -100.0                                          # a flushed magnitude
    x[B - 1, K - 1, NB + 2, Fr // 3] = 1500.0                             # inside the 1608 rad polar() documents
    x64 = x.double()
    inp = {"x": x.reshape(B, K * 2 * NB, Fr).contiguous(),
           "x_pre": torch.cat([(x64[:, :, :NB] * LOG2E).float(), (x64[:, :, NB:] * INV2PI).float()], 2).reshape(B, K * 2 * NB, Fr).contiguous(),
           "spec": torch.exp(x64[:, :, :NB]).float().contiguous(),
           "phase": (math.pi * torch.sin(x64[:, :, NB:])).float().contiguous(),
           "filt": 0.1 * torch.randn(4, 63, generator=g)}
    return inp


def tail_inputs(c):
    return _inputs(c["name"].split("/")[0])


def bank_of(c, inp):
    return torch.from_numpy(R.pqmf_synthesis_filter(4)) if c["bank"] == "fixed" else inp["filt"]


# ---------------------------------------------------------------------------------------------- the restatement
def _basis(dtype, exact):
    n = torch.arange(N_FFT, dtype=F64)[:, None]
    k = torch.arange(NB, dtype=F64)[None, :]
    ang = 2 * math.pi * n * k / N_FFT
    if not exact:
        Cm, Sm = R._idft_basis(N_FFT)
        return Cm.to(dtype), Sm.to(dtype), ang
    scale = torch.full((1, NB), 2.0, dtype=F64)
    scale[0, 0] = scale[0, -1] = 1.0
    Sm = -scale * torch.sin(ang) / N_FFT
    Sm[:, 0] = Sm[:, -1] = 0.0
    return (scale * torch.cos(ang) / N_FFT).to(dtype), Sm.to(dtype), ang


def _window(dtype, exact, mut=None):
    n = np.arange(N_FFT)
    if mut == "hann_sym":
        w = 0.5 - 0.5 * np.cos(2 * np.pi * n / (N_FFT - 1))
    else:
        w = 0.5 - 0.5 * np.cos(2 * np.pi * n / N_FFT)
    return torch.from_numpy(w if exact else w.astype(np.float32)).to(dtype)


def _irfft16_packed(re, im, dtype, exact):
    """irfft16_hann of csrc/istft_pqmf.hip, operation for operation: [B, K, 9, F] -> windowed frames [B, K, 16, F]."""
    j = np.arange(N_FFT)
    c16, s16, hann = np.cos(2 * np.pi * j / N_FFT), np.sin(2 * np.pi * j / N_FFT), 0.5 - 0.5 * np.cos(2 * np.pi * j / N_FFT)
    if not exact:
        c16, s16, hann = (a.astype(np.float32) for a in (c16, s16, hann))
    k_ = lambda a: [torch.tensor(float(v), dtype=dtype) for v in a]
    C16, S16, H = k_(c16), k_(s16), k_(hann / 16)
    r, i = [re[:, :, k] for k in range(NB)], [im[:, :, k] for k in range(NB)]
    Z = [None] * 8
    Z[0] = (r[0] + r[8], r[0] - r[8])
    Z[4] = (2 * r[4], -2 * i[4])
    for k in range(1, 4):
        Ar, Ai, Dr, Di = r[k] + r[8 - k], i[k] - i[8 - k], r[k] - r[8 - k], i[k] + i[8 - k]
        Br, Bi = -S16[k] * Dr - C16[k] * Di, C16[k] * Dr - S16[k] * Di
        Z[k], Z[8 - k] = (Ar + Br, Ai + Bi), (Ar - Br, Bi - Ai)

    def idft4(y0, y1, y2, y3):
        t0, t1 = (y0[0] + y2[0], y0[1] + y2[1]), (y0[0] - y2[0], y0[1] - y2[1])
        t2, t3 = (y1[0] + y3[0], y1[1] + y3[1]), (y1[0] - y3[0], y1[1] - y3[1])
        return [(t0[0] + t2[0], t0[1] + t2[1]), (t1[0] - t3[1], t1[1] + t3[0]), (t0[0] - t2[0], t0[1] - t2[1]), (t1[0] + t3[1], t1[1] - t3[0])]
    E, O = idft4(Z[0], Z[2], Z[4], Z[6]), idft4(Z[1], Z[3], Z[5], Z[7])
    rt = torch.tensor(math.sqrt(0.5) if exact else float(np.float32(math.sqrt(0.5))), dtype=dtype)
    T = [O[0], ((O[1][0] - O[1][1]) * rt, (O[1][0] + O[1][1]) * rt), (-O[2][1], O[2][0]), ((-O[3][0] - O[3][1]) * rt, (O[3][0] - O[3][1]) * rt)]
    out = [None] * N_FFT
    for n in range(4):
        a, b = (E[n][0] + T[n][0], E[n][1] + T[n][1]), (E[n][0] - T[n][0], E[n][1] - T[n][1])
        out[2 * n], out[2 * n + 1], out[2 * n + 8], out[2 * n + 9] = a[0] * H[2 * n], a[1] * H[2 * n + 1], b[0] * H[2 * n + 8], b[1] * H[2 * n + 9]
    return torch.stack(out, 2)


def _ola(fr):
    """[..., 16, F] -> [..., 4 (F - 1)]: overlap-add at hop 4, n_fft / 2 trimmed on each side."""
    Fr = fr.shape[-1]
    total = N_FFT + HOP * (Fr - 1)
    out = torch.zeros(*fr.shape[:-2], total, dtype=fr.dtype)
    for n in range(N_FFT):
        out[..., n:n + HOP * (Fr - 1) + 1:HOP] += fr[..., n, :]
    return out[..., N_FFT // 2:total - N_FFT // 2]


def _stuff(y, gain=4.0, phase=0):
    up = torch.zeros(*y.shape[:-1], y.shape[-1] * 4, dtype=y.dtype)
    up[..., phase::4] = y * gain
    return up


def _synth(up, h, pad=(31, 31)):
    return F.conv1d(F.pad(up, pad), h.view(1, h.shape[0], -1))


def _fn32(f, x):
    """A correctly rounded fp32 function of an fp32 argument."""
    return f(x.double()).float()


def _polar(c, inp, dtype, mut, style):
    B, K, Fr = c["B"], c["K"], c["F"]
    v = c["variant"]
    turns = style == "turns"
    assert not turns or dtype == F32
    if v == "polar":
        spec, phase = inp["spec"].to(dtype), inp["phase"].to(dtype)
        if turns:
            t = phase * np.float32(INV2PI)
            return spec, phase, spec * _fn32(lambda a: torch.cos(2 * math.pi * a), t), spec * _fn32(lambda a: torch.sin(2 * math.pi * a), t)
        return spec, phase, spec * torch.cos(phase), spec * torch.sin(phase)
    pre = v == "pre" and mut != "prescale_ignored"
    x = inp["x_pre" if v == "pre" else "x"].to(dtype).view(B, K, 2 * NB, Fr)
    xm, xp = x[:, :, :NB], x[:, :, NB:]
    pi = math.pi if mut != "phase_no_pi" else 1.0
    if turns:
        spec = _fn32(torch.exp2, xm if pre else xm * np.float32(LOG2E))
        s = _fn32(lambda a: torch.sin(2 * math.pi * a), xp if pre else xp * np.float32(INV2PI))
        phase = np.float32(pi) * s
        half = 0.5 * s if mut != "phase_no_pi" else s * np.float32(INV2PI)
        return spec, phase, spec * _fn32(lambda a: torch.cos(2 * math.pi * a), half), spec * _fn32(lambda a: torch.sin(2 * math.pi * a), half)
    if pre and dtype == F64:
        spec, phase = torch.exp2(xm), pi * torch.sin(2 * math.pi * xp)
    elif pre:                                  # the exact-math route's own scaling back (polar<false, true>)
        spec, phase = torch.exp(xm * np.float32(math.log(2.0))), np.float32(pi) * torch.sin(xp * np.float32(2 * math.pi))
    else:
        spec, phase = torch.exp(xm), pi * torch.sin(xp)
    return spec, phase, spec * torch.cos(phase), spec * torch.sin(phase)


def tail_compute(c, inp, dtype, mut=None, style="plain"):
    """-> spec, phase [B, K, 9, F] (the inputs themselves for `polar`), omb, o, and the intermediates of the bound."""
    exact = dtype == F64
    spec, phase, re, im = _polar(c, inp, dtype, mut, style)
    Cm, Sm, _ = _basis(dtype, exact)
    if style == "packed":
        assert mut is None
        fr = _irfft16_packed(re, im, dtype, exact)
    else:
        fr = torch.einsum("nk,bckf->bcnf", Cm, re) + torch.einsum("nk,bckf->bcnf", Sm, im)
    if mut == "dc_imag":
        fr = fr + im[:, :, 0:1] * torch.tensor([-1.0, 1.0] * 8, dtype=dtype)[None, None, :, None] / N_FFT
    if mut == "nyq_imag":
        fr = fr - im[:, :, 8:9] / N_FFT
    if style != "packed":
        fr = fr * _window(dtype, exact, mut)[None, None, :, None]
    wsq = (_window(dtype, exact) ** 2)[:, None].expand(N_FFT, c["F"]).clone()
    if mut == "env_last_frame":
        wsq[:, -1] = 0
    env = _ola(wsq)
    if mut == "wsq_7_9":                         # the edge table's entries 7 and 9 off by 2e-6 (the interior is the constant 1.5)
        wsq[7], wsq[9] = 0.92533011387037270, 0.92533011387037270
        quad = torch.arange(env.shape[-1]) // HOP
        env = torch.where((quad >= 1) & (quad + 2 < c["F"]), env, _ola(wsq))
    if mut == "env_flat":
        env = torch.full_like(env, 1.5)
    y = _ola(fr) * (1 / env) if style == "packed" else _ola(fr) / env                                                      # [B, K, 4 (F - 1)]
    out = {"spec": spec, "phase": phase, "re": re, "im": im, "fr": fr, "env": env, "y": y}
    if c["kind"] == "sb":
        out["o"] = y
        return out
    h = bank_of(c, inp).to(dtype)
    if mut in ("tap0", "tap62"):
        h = h.clone()
        h[:, 0 if mut == "tap0" else 62] = 0
    if mut == "band_swap":
        h = h[[0, 2, 1, 3]]
    if mut == "trainable_reversed" and c["bank"] == "trainable":
        h = h.flip(-1)
    up = _stuff(y, 1.0 if mut == "no_gain4" else 4.0, 1 if mut == "stuff_phase" else 0)
    out["omb"] = up if c["layout"] == "ms" else y
    pad = (30, 32) if mut == "pad_30_32" else (31, 31)
    if mut == "halo_zero":                       # every 480-tile filters only its own sub-band samples
        o = torch.zeros(c["B"], 1, up.shape[-1], dtype=dtype)
        for m0 in range(0, y.shape[-1], 480):
            own = torch.zeros_like(up)
            own[..., 4 * m0:4 * (m0 + 480)] = up[..., 4 * m0:4 * (m0 + 480)]
            o[..., 4 * m0:4 * (m0 + 480)] = _synth(own, h, pad)[..., 4 * m0:4 * (m0 + 480)]
        out["o"] = o
    else:
        out["o"] = _synth(up, h, pad)
    return out


def tail_bound(c, inp, ref):
    """A (float64, in units of u) for spec, phase, omb and o; see the module docstring."""
    B, K, Fr = c["B"], c["K"], c["F"]
    spec, ph, re, im = ref["spec"], ref["phase"], ref["re"], ref["im"]
    A = {}
    if c["variant"] == "polar":
        E_mag, E_ang = torch.zeros_like(spec), 2 * ph.abs()                  # ph / (2 pi): the constant, the product
    else:
        x = inp["x_pre" if c["variant"] == "pre" else "x"].double().view(B, K, 2 * NB, Fr)
        xm, xp = x[:, :, :NB], x[:, :, NB:]
        if c["variant"] == "pre":
            xm, xp = xm * math.log(2.0), xp * 2 * math.pi
        s = torch.sin(xp)
        E_mag = spec * (2 * xm.abs() + 1)                                    # x log2e: the constant, the product; the exp
        E_s = 2 * xp.abs() * torch.cos(xp).abs() + s.abs()                   # x / 2 pi: the constant, the product; the sine
        E_ang = math.pi * E_s + 2 * ph.abs()                                 # pi s: the constant, the product
        A["spec"], A["phase"] = E_mag, E_ang
    cs, sn = torch.cos(ph).abs(), torch.sin(ph).abs()
    E_re = E_mag * cs + spec * (sn * E_ang + cs) + re.abs()
    E_im = E_mag * sn + spec * (cs * E_ang + sn) + im.abs()
    Cm, Sm, _ = _basis(F64, True)
    scale = torch.full((NB,), 2.0, dtype=F64)
    scale[0] = scale[-1] = 1.0
    lin = torch.einsum("nk,bckf->bcnf", Cm.abs(), E_re) + torch.einsum("nk,bckf->bcnf", Sm.abs(), E_im)
    G = ((re.abs() + im.abs()) * scale[None, None, :, None]).sum(2, keepdim=True) / N_FFT
    A_fr = _window(F64, True)[None, None, :, None] * (lin + DEPTH * G)
    A_y = (_ola(A_fr) + 3 * _ola(ref["fr"].abs())) / ref["env"] + 6 * ref["y"].abs()
    if c["kind"] == "sb":
        A["o"] = A_y
        return A
    A["omb"] = _stuff(A_y) if c["layout"] == "ms" else A_y
    A["o"] = _synth(_stuff(A_y + NK[c["bank"]] * ref["y"].abs()), bank_of(c, inp).double().abs())
    return A


@functools.lru_cache(maxsize=None)
def _shared(name, variant, bank, layout):
    c = with_variant(next(x for x in TAIL_CASES if x["name"] == name), variant, bank, layout)
    inp = tail_inputs(c)
    ref = tail_compute(c, inp, F64)
    return inp, ref, tail_bound(c, inp, ref), {s: tail_compute(c, inp, F32, style=s) for s in STYLES}


def tail_shared(c):
    """Inputs, float64 reference, bound and the fp32 oracles of a run, computed once and left unchanged.  A run with a
    `filt` of its own (a net's trainable bank instead of the case's) is computed on the spot."""
    if c.get("filt") is None:
        return _shared(c["name"].split("/")[0], c["variant"], c["bank"], c["layout"])
    inp = dict(tail_inputs(c), filt=c["filt"])
    ref = tail_compute(c, inp, F64)
    return inp, ref, tail_bound(c, inp, ref), {s: tail_compute(c, inp, F32, style=s) for s in STYLES}


# ---------------------------------------------------------------------------------------------- the bars
def check_rounded(kernel, what, got, ref, A, orcs, tol_scale=1.0, margin=MARGIN, stats=None):
    """small_op_cases.check_rounded with the quantile bars taken from the larger of several fp32 oracles."""
    if len(orcs) == 1:
        return sc.check_rounded(kernel, what, got, ref, A, orcs[0], tol_scale=tol_scale, margin=margin, stats=stats)
    got = got.to(F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(ref).all()), (what, "reference not finite")
    assert bool(torch.isfinite(got).all()), (what, "non-finite output", int((~torch.isfinite(got)).sum()))
    err = (got - ref).abs()
    tol = TOL[kernel] * tol_scale
    ratio = float(((err - FLOOR).clamp_min(0) / (U * A).clamp_min(1e-300)).max())
    bad = err > tol * U * A + FLOOR
    ulp = ulp32(float(ref.pow(2).mean().sqrt()))
    q = lambda e, p: float(torch.quantile(e.flatten()[:: max(1, e.numel() // 4000000)], p))
    med, p999 = q(err, 0.5), q(err, 0.999)
    med_o = max(q((o.to(F64) - ref).abs(), 0.5) for o in orcs)
    p999_o = max(q((o.to(F64) - ref).abs(), 0.999) for o in orcs)
    if stats is not None:
        stats.add(kernel, ratio, med / (margin * med_o + ulp), p999 / (margin * p999_o + ulp))
    print("%-40s err/(uA) %.3g (tol %.3g)  median %.3g (oracles %.3g)  p99.9 %.3g (oracles %.3g)  ulp(rms) %.3g"
          % (what, ratio, tol, med, med_o, p999, p999_o, ulp))
    assert not bool(bad.any()), (what, "element bar", int(bad.sum()), float(err.max()), ratio, tol)
    assert med <= margin * med_o + ulp, (what, "median", med, med_o, ulp)
    assert p999 <= margin * p999_o + ulp, (what, "p99.9", p999, p999_o, ulp)


def tail_check(c, got, styles=("plain",), **kw):
    """got: the outputs present among spec, phase, omb, o (fp32, any shape with the reference's element order);
    styles: the fp32 oracles whose errors set the quantile bars (exact-math route: plain; hardware route: both)."""
    inp, ref, A, orcs = tail_shared(c)
    for k in ("spec", "phase", "omb", "o"):
        if k in got:
            assert k in A, (c["name"], k, "no such output in this variant")
            check_rounded("tail_" + k, c["name"] + " " + k, got[k].reshape(ref[k].shape), ref[k], A[k],
                          [orcs[s][k] for s in styles], **kw)
