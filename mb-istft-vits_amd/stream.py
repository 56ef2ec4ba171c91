"""Streaming decode: the waveform of `dec(z, g)[0]` chunk by chunk, bitwise equal to the one-shot decode.

The decoder is not recurrent and its receptive field is finite: any sample of z-frame t depends on z-frames
[t - L, t + R] only (`decoder_context`).  A chunk [first, first + count) is decoded from the z-window
[first - L, first + count + R) clipped to the utterance, and only the chunk's own samples are stored, in place, in
the caller's full-length output (`mbv_decode_range`).  The window's edges are padded with zeros exactly as a
stand-alone decode pads its own; what that changes lies within L / R of a window edge, and those samples belong
to other chunks.  Every conv of the window runs the same chain of operations as the conv of the whole utterance,
so in the default mode the kept samples are bitwise the one-shot samples.

Chunk sizes double from `chunk_frames` up to `max_chunk_frames` (`chunk_schedule`): a small first chunk keeps the
time to the first audio low, and the halo cost (L + R frames of decoder work per chunk) is paid O(log T') times.

Many streams at once: a `StreamPool` decodes the next chunk of each of its streams in ONE call (`mbv_decode_chunks`),
one decoder run per class of utterance lengths instead of one launch chain per stream, every sample bitwise what the
stream yields alone.

Audio that is still arriving: a `LiveStream` (`net.convert_live`) takes a recording in `push` calls, converts z_hat
frames from spectrogram windows as soon as the samples they depend on exist (`LivePlan`, `mbv_convert_ranges`) and
decodes every chunk whose z-window is final; a `StreamPool` serves live streams next to finished ones.

A live call cannot wait for the full reach of the layers: `Ahead(conv, dec)` bounds how far a block of z_hat frames and
a decoder chunk look to their right, on a fixed grid, so that the result is still a pure function of the recording
(opt-in, an approximation with an exact definition: DESIGN §7.25).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi


def chunk_schedule(t_frames, chunk_frames=32, max_chunk_frames=256):
    """[(first, count), ...] covering [0, t_frames) once, in order: counts chunk_frames, 2 chunk_frames, ...
    capped at max_chunk_frames, the last one cut at t_frames.  Pure function of its arguments."""
    t_frames, c, cap = int(t_frames), int(chunk_frames), int(max_chunk_frames)
    if t_frames < 0:
        raise ValueError("t_frames must be >= 0")
    if c < 1 or cap < c:
        raise ValueError("need 1 <= chunk_frames <= max_chunk_frames (got %d, %d)" % (c, cap))
    out, first = [], 0
    while first < t_frames:
        n = min(c, t_frames - first)
        out.append((first, n))
        first += n
        c = min(2 * c, cap)
    return out


RES_TYPES = _capi.RESAMPLE_TYPES    # MBV_RESAMPLE_KAISER_*: the filters of the warp and the wire


def frame_rates(pitch, marks, frames, glide_frames=2):
    """The rate table of a pitched utterance, fp32 [frames] on the host: frame f takes the pitch of the
    token that holds it (`marks`: the frame at which every token starts, the last entry the end; 1.0 for a frame no
    token holds), then the glide: the float64 mean over [f - g, f + g] within [0, frames), added in ascending order and
    rounded to fp32.  glide_frames = 0 keeps the steps."""
    g = int(glide_frames)
    if g < 0:
        raise ValueError("pitch_glide_frames must be >= 0, got %d" % g)
    step = np.ones(int(frames), np.float32)
    for j, p in enumerate(pitch):
        step[min(int(marks[j]), frames):min(int(marks[j + 1]), frames)] = np.float32(p)
    if g == 0:
        return step
    vals = [float(v) for v in step]
    out = np.empty_like(step)
    for f in range(len(vals)):
        lo, hi = max(0, f - g), min(len(vals), f + g + 1)
        acc = 0.0
        for k in range(lo, hi):
            acc += vals[k]
        out[f] = np.float32(acc / float(hi - lo))
    return out


class WarpMap:
    """The time warp of one pitched utterance: `rate` fp32 [F], the playback rate of every kept z-frame,
    `U` float64 [F + 1], the warped position of every frame start (`mbv_warp_plan`: U[f + 1] = U[f] + hop / rate[f]),
    and `n_out` = floor(U[F]), the warped length.  Both tables live on the host (`rate`, `U`: NumPy) and, once `device`
    is given, on the device (`rate_dev`, `U_dev`: uploaded once).  The C side is the authority for every number here."""

    __slots__ = ("rate", "U", "n_out", "hop", "frames", "rate_dev", "U_dev")

    def __init__(self, rate, hop, device=None):
        rate = np.ascontiguousarray(rate, np.float32).reshape(-1)
        hop = int(hop)
        U = np.empty(len(rate) + 1, np.float64)
        n_out = C.c_int64()
        L = _capi.lib()
        if L.mbv_warp_plan(hop, len(rate), rate.ctypes.data, U.ctypes.data, C.byref(n_out)):
            raise ValueError((L.mbv_last_error(None) or b"mbv_warp_plan failed").decode())
        self.rate, self.U, self.n_out, self.hop, self.frames = rate, U, int(n_out.value), hop, len(rate)
        self.rate_dev = self.U_dev = None
        if device is not None:
            self.rate_dev = torch.from_numpy(rate).to(device)
            self.U_dev = torch.from_numpy(U).to(device)

    def __repr__(self):
        return "WarpMap(%d frames of %d samples -> %d samples)" % (self.frames, self.hop, self.n_out)

    @property
    def samples(self):
        return self.frames * self.hop

    def ready(self, in_avail, res_type="kaiser_best"):
        """Warped samples that are final once the model samples [0, in_avail) exist (`mbv_warp_ready`)."""
        n = _capi.lib().mbv_warp_ready(self.hop, self.frames, self.rate.ctypes.data, self.U.ctypes.data,
                                       _res_code(res_type), int(in_avail))
        if n < 0:
            raise ValueError((_capi.lib().mbv_last_error(None) or b"mbv_warp_ready failed").decode())
        return int(n)

    def samples_of_frames(self, frames):
        """ceil(U[f]) of every z-frame index (clipped to the map's frames): the first warped sample at or behind the
        frame's first model sample, as integers."""
        return [int(math.ceil(self.U[min(max(int(f), 0), self.frames)])) for f in frames]


def _res_code(res_type):
    if res_type not in RES_TYPES:
        raise ValueError("res_type must be 'kaiser_best' or 'kaiser_fast', got %r" % (res_type,))
    return RES_TYPES[res_type]


def decoder_context(config_struct):
    """(L, R) of `mbv_decoder_context` for an `_capi.MbvConfig` (host only)."""
    out = (C.c_int32 * 2)()
    if _capi.lib().mbv_decoder_context(C.byref(config_struct), C.byref(out)):
        raise _capi.MbvError("mbv_decoder_context: unsupported decoder %d" % config_struct.decoder)
    return int(out[0]), int(out[1])


def converter_context(config_struct):
    """(L, R) of `mbv_converter_context` for an `_capi.MbvConfig` (host only): z_hat frame t depends on spectrogram
    frames [t - L, t + R] only."""
    out = (C.c_int32 * 2)()
    if _capi.lib().mbv_converter_context(C.byref(config_struct), C.byref(out)):
        raise _capi.MbvError("mbv_converter_context failed")
    return int(out[0]), int(out[1])


def spectrogram_ready(arrived, closed, n_fft, hop_size):
    """Leading spectrogram frames that are final once `arrived` samples exist (`mbv_spectrogram_ready`, host only)."""
    r = int(_capi.lib().mbv_spectrogram_ready(int(arrived), int(bool(closed)), int(n_fft), int(hop_size)))
    if r < 0:
        raise ValueError("mbv_spectrogram_ready refused (arrived %d, n_fft %d, hop_size %d)" % (arrived, n_fft, hop_size))
    return r


def check_closable(arrived, sr, n_fft, hop_size):
    """A recording may be closed once it gives a spectrogram frame; ValueError otherwise (the one check of
    `LiveStream.close` and `wire.LiveWirePlan.close`; `arrived` counts samples at the model's rate `sr`)."""
    if arrived < 1 or spectrogram_ready(arrived, True, n_fft, hop_size) < 1:
        raise ValueError("%d samples at %d Hz give no spectrogram frame (n_fft %d, hop_size %d)"
                         % (arrived, sr, n_fft, hop_size))


def _decode_chunks(net, work):
    """One decoder call for `work` = [(stream, first, count), ...], each a chunk its stream is ready for: the streams
    fill the `MbvChunk` table (`_fill_chunk`) and are told what was decoded (`_chunk_decoded`).  A member that names
    a route length (a recording that is still growing) makes it `mbv_decode_chunks_routed`.  Members with a seam
    (`Ahead(seam_ms=)`, at most one chunk of each in `work`) then share ONE `mbv_seam_rows` launch."""
    arr = (_capi.MbvChunk * len(work))()
    route = (C.c_int32 * len(work))()
    for i, (st, first, count) in enumerate(work):
        route[i] = st._fill_chunk(arr[i], first, count) or 0
    if any(route):
        net._call("mbv_decode_chunks_routed", arr, route, len(work))
    else:
        net._call("mbv_decode_chunks", arr, len(work))
    seams = [w for w in work if getattr(w[0], "seam", 0)]
    if seams:
        rows = (_capi.MbvSeamRow * len(seams))()
        if sum(st._fill_seam(row, first, count) for row, (st, first, count) in zip(rows, seams)):
            net._call("mbv_seam_rows", rows, len(seams))
    for st, first, count in work:
        st._chunk_decoded(first, count)


def _convert_ranges(net, todo, hop_size, win_size):
    """One `mbv_convert_ranges` run for `todo` = [(live stream, (a, b)), ...], a z_hat range due on each; with a member
    of a bounded look-ahead among them (whose grid blocks may be several rows) it is `mbv_convert_ranges_ahead`, the
    other members at the full reach."""
    rows = (_capi.MbvConvertRange * len(todo))()
    for row, (st, due) in zip(rows, todo):
        st._fill_range(row, *due)
    if any(st._plan.ahead is not None for st, _ in todo):
        ahead = (C.c_int32 * len(todo))(*[st._plan.conv_ahead for st, _ in todo])
        net._call("mbv_convert_ranges_ahead", rows, ahead, len(todo), hop_size, win_size)
    else:
        net._call("mbv_convert_ranges", rows, len(todo), hop_size, win_size)
    for st, due in todo:
        st._plan.converted(*due)


def _convert_live(net, members):
    """The z_hat ranges due on every live stream among `members` (the grid blocks of a bounded one are several), in one
    `mbv_convert_ranges` run per run of the planner."""
    by_cfg = {}
    for st in members:
        for due in st._due_blocks():
            st._check_handle()
            by_cfg.setdefault((st.hop_size, st.win_size), []).append((st, due))
    L = _capi.lib()
    for (hop, win), todo in by_cfg.items():
        n = len(todo)
        wl = (C.c_int32 * n)(*[st._window_frames(*due) for st, due in todo])
        run_of = (C.c_int32 * n)()
        n_runs = L.mbv_convert_ranges_plan(C.byref(todo[0][0]._cfg_struct), n, wl, run_of)
        if n_runs < 1:
            raise ValueError("mbv_convert_ranges_plan refused the windows (one beyond the fused WN layers?)")
        for r in range(n_runs):
            _convert_ranges(net, [t for t, k in zip(todo, run_of) if k == r], hop, win)


class Ahead:
    """A bounded look-ahead of a live stream: a block of z_hat frames is converted from a spectrogram
    window that ends `conv` frames behind it (0 <= conv <= R_conv of `converter_context`), a chunk is decoded from the
    z_hat frames up to `dec` behind it (0 <= dec <= R_dec of `decoder_context`).  `seam_ms` > 0 cross-fades the first
    round(seam_ms * model_sr / 1000) samples of every chunk with what the previous decode gave for them (5 ms is a
    sensible value: a convention, not a measurement).  `Ahead(R_conv, R_dec)` is bitwise the stream without it."""

    __slots__ = ("conv", "dec", "seam_ms")

    def __init__(self, conv, dec, seam_ms=0.0):
        for name, v in (("conv", conv), ("dec", dec)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError("Ahead: %s must be an integer number of frames, got %r" % (name, v))
            if v < 0:
                raise ValueError("Ahead: %s must be >= 0, got %d" % (name, v))
        if isinstance(seam_ms, bool) or not isinstance(seam_ms, (int, float, np.integer, np.floating)):
            raise TypeError("Ahead: seam_ms must be a number of milliseconds, got %r" % (seam_ms,))
        if not math.isfinite(seam_ms) or seam_ms < 0:
            raise ValueError("Ahead: seam_ms must be finite and >= 0, got %r" % (seam_ms,))
        self.conv, self.dec, self.seam_ms = int(conv), int(dec), float(seam_ms)

    def __repr__(self):
        return "Ahead(%d, %d%s)" % (self.conv, self.dec, ", seam_ms=%g" % self.seam_ms if self.seam_ms else "")

    def seam_samples(self, model_sr):
        """S = round(seam_ms * model_sr / 1000) (0 without a seam)."""
        return int(round(self.seam_ms * int(model_sr) / 1000.0)) if self.seam_ms else 0


class LivePlan:
    """What a recording that is still arriving may convert and decode, in pure integers (no tensor, no GPU).

      spectrogram frame f   final iff closed, or all its samples exist               (`spectrogram_ready`)
      z_hat frame t         may be converted iff spectrogram frames up to t + R_conv are final, or closed
      conversion            launches when >= `convert_frames` new z_hat frames may be converted, or on close
      chunk (first, count)  decodable iff z_hat frames up to first + count + R_dec are converted, or closed
    Chunks are those of `chunk_schedule(T, chunk_frames, max_chunk_frames)`: only the cut of the last one depends on T,
    and while the recording is open a decodable chunk lies R_dec frames before the end, so it is never the cut one.

    With `ahead=Ahead(conv, dec)` conversion runs on a fixed grid instead, cf = `convert_frames`:
      block k               z_hat frames [k cf, min((k + 1) cf, T)), converted from the spectrogram window that ends at
                            E_k = min((k + 1) cf + conv, T); due iff E_k frames are final, or closed.  `convert_due()`
                            returns the list of all blocks due (possibly empty)
      chunk (first, count)  decoded with t_frames = D = min(first + count + dec, T) (`t_frames`), decodable iff z_hat
                            frames up to D are converted
      seam                  S samples (`seam`, needs `model_sr` and `samples_per_frame`): the chunk is decoded
                            `overhang(first, count)` = min(ceil(S / spf), D - first - count) frames past its end
    so that what is converted and decoded, and from what, does not depend on the pushes."""

    def __init__(self, n_fft, hop_size, r_conv, r_dec, chunk_frames=32, max_chunk_frames=256, convert_frames=32,
                 ahead=None, model_sr=None, samples_per_frame=None):
        self.n_fft, self.hop = int(n_fft), int(hop_size)
        self.r_conv, self.r_dec = int(r_conv), int(r_dec)
        c, cap, cf = int(chunk_frames), int(max_chunk_frames), int(convert_frames)
        if c < 1 or cap < c:
            raise ValueError("need 1 <= chunk_frames <= max_chunk_frames (got %d, %d)" % (c, cap))
        if cf < 1:
            raise ValueError("convert_frames must be >= 1")
        self.convert_frames = cf
        self.ahead, self.seam, self._over_frames = ahead, 0, 0
        if ahead is not None:
            if not isinstance(ahead, Ahead):
                raise TypeError("ahead must be a stream.Ahead or None, got %r" % (ahead,))
            if ahead.conv > self.r_conv or ahead.dec > self.r_dec:
                raise ValueError("%r looks further than the model can: conv <= %d, dec <= %d" % (ahead, self.r_conv, self.r_dec))
            if ahead.seam_ms:
                if model_sr is None or samples_per_frame is None:
                    raise ValueError("a seam needs model_sr and samples_per_frame")
                S, spf = ahead.seam_samples(model_sr), int(samples_per_frame)
                if not 1 <= S <= spf * min(ahead.dec, c):
                    raise ValueError("a seam of %g ms is %d samples at %d Hz: it must be 1 .. %d, the samples of the dec = %d "
                                     "frames a chunk looks ahead and of the smallest chunk (%d frames)"
                                     % (ahead.seam_ms, S, int(model_sr), spf * min(ahead.dec, c), ahead.dec, c))
                self.seam, self._over_frames = S, -(-S // spf)
        self.arrived, self.closed = 0, False
        self.z_done = 0                        # z_hat frames [0, z_done) are converted
        self._first, self._c, self._cap = 0, c, cap          # the next chunk to release
        self._c0 = c

    def push(self, n):
        if self.closed:
            raise ValueError("push after close()")
        self.arrived += int(n)

    def close(self):
        self.closed = True

    @property
    def spec_final(self):
        return spectrogram_ready(self.arrived, self.closed, self.n_fft, self.hop)

    @property
    def total(self):
        """T, once closed."""
        return self.spec_final if self.closed else None

    @property
    def conv_ahead(self):
        """Frames a converted range looks to its right: `ahead.conv`, else R_conv."""
        return self.r_conv if self.ahead is None else self.ahead.conv

    @property
    def dec_ahead(self):
        return self.r_dec if self.ahead is None else self.ahead.dec

    def due_blocks(self):
        """[(a, b), ...]: every z_hat range to convert now, in order (one at most without `ahead`)."""
        if self.ahead is None:
            due = self.convert_due()
            return [] if due is None else [due]
        f, cf, a, out = self.spec_final, self.convert_frames, self.z_done, []
        while True:
            if self.closed:
                if a >= f:
                    break
                b = min(a + cf, f)
            else:
                b = a + cf
                if b + self.ahead.conv > f:
                    break
            out.append((a, b))
            a = b
        return out

    def convert_due(self):
        """The z_hat range [a, b) to convert now, or None.  With `ahead`: the list of the grid blocks due now."""
        if self.ahead is not None:
            return self.due_blocks()
        f = self.spec_final
        b = f if self.closed else max(0, f - self.r_conv)
        a = self.z_done
        if b > a and (self.closed or b - a >= self.convert_frames):
            return a, b
        return None

    def converted(self, a, b):
        if a != self.z_done or b <= a:
            raise ValueError("ranges are converted in order, once")
        self.z_done = b

    def decodable(self):
        """[(first, count), ...]: the chunks not released yet that are decodable now, in order."""
        first, c, out = self._first, self._c, []
        T = self.spec_final if self.closed else None
        while True:
            if self.ahead is not None:         # z_hat up to the chunk's D (of the uncut chunk while T is not known)
                if self.closed and first >= T:
                    break
                n = min(c, T - first) if self.closed else c
                if self.z_done < self.t_frames(first, n):
                    break
            elif self.closed:
                if self.z_done < T or first >= T:
                    break
                n = min(c, T - first)
            else:
                if self.z_done < first + c + self.r_dec:
                    break
                n = c
            out.append((first, n))
            first, c = first + n, min(2 * c, self._cap)
        return out

    def t_frames(self, first, count):
        """D of chunk (first, count): the z_hat frames [0, D) it is decoded from, min(first + count + dec, T) (T once
        closed; a chunk decodable before lies wholly inside the recording).  Without `ahead`: what is converted."""
        if self.ahead is None:
            return self.z_done
        D = first + count + self.ahead.dec
        return min(D, self.spec_final) if self.closed else D

    def overhang(self, first, count):
        """Frames chunk (first, count) is decoded past its end for the seam (0 without one)."""
        return min(self._over_frames, self.t_frames(first, count) - first - count) if self.seam else 0

    def lag(self):
        """(arrived, frames): the sample count at which the first chunk is released when `poll()` follows every push
        however small, and the steady-state lag: the largest distance, over the chunks of full size, from a chunk's
        first frame to the number of final spectrogram frames its release waits for.  Pure integers; without `ahead`
        the same arithmetic at (R_conv, R_dec), which the unbounded stream meets under such pushes."""
        cf, conv, dec = self.convert_frames, self.conv_ahead, self.dec_ahead
        need = lambda first, c: -(-(first + c + dec) // cf) * cf + conv     # final frames chunk (first, c) waits for
        first, c, cap = 0, self._c0, self._cap
        arrived = (need(0, c) - 1) * self.hop + self.n_fft - (self.n_fft - self.hop) // 2
        steady, seen = 0, 0
        while seen < cf:
            if c == cap:
                steady, seen = max(steady, need(first, c) - first), seen + 1
            first, c = first + c, min(2 * c, cap)
        return arrived, steady

    def next_chunk(self):
        """The next chunk (first, count) if it is decodable now, else None."""
        d = self.decodable()
        return d[0] if d else None

    def released(self, first, count):
        if first != self._first:
            raise ValueError("chunks are released in order")
        self._first += count
        self._c = min(2 * self._c, self._cap)

    @property
    def all_released(self):
        return self.closed and self._first >= self.spec_final


class LiveStream:
    """Voice conversion of a recording that is pushed piece by piece (`net.convert_live`).

    `push(samples)` appends to a device buffer allocated once; `poll()` converts the z_hat frames whose audio exists
    (one `mbv_convert_ranges` run over a spectrogram window, only the new frames stored into the stream's own `z`),
    decodes every chunk that has become decodable and returns `[(first_sample, view), ...]`; `close()` ends the
    recording.  z, o, g, the noise block and the sample buffer belong to the stream, so `infer`, `voice_conversion`
    or other streams may run between any two calls.  Once `finished`, `y_lengths` is set and `result()` is
    o[:, :, :256 T].  A `StreamPool` converts and decodes for many live streams in shared launches; chunks it decoded
    ahead are handed out by the next `poll()` without a launch.

    `ahead=Ahead(conv, dec, seam_ms)` (opt-in) bounds the look-ahead for a call that is live: conversion on
    the fixed grid of `convert_frames`, every chunk decoded with its canonical t_frames, the first `seam` samples of a
    chunk cross-faded with the previous decode's overhang (`mbv_seam_rows`).  Still a pure function of the recording;
    an approximation of the stream without `ahead`, which `Ahead(R_conv, R_dec)` is bitwise."""

    def __init__(self, net, sid_src, sid_tgt, model_sr, hop_size, win_size, max_samples, dtype=torch.float32,
                 noise_scale=1.0, noise=None, chunk_frames=32, max_chunk_frames=256, convert_frames=32, in_sr=None,
                 seed=None, ahead=None):
        import math
        if seed is not None:
            from .models import _row_seeds
            if noise is not None:
                raise ValueError("convert_live: seed= and noise= exclude each other")
            seed = _row_seeds(seed, 1, "convert_live: seed")[0][0]
        self.model_sr, self.hop_size, self.win_size = int(model_sr), int(hop_size), int(win_size)
        if in_sr is not None and int(in_sr) != self.model_sr:
            raise ValueError("convert_live takes audio at the model's rate (in_sr %d, model_sr %d): a streaming input "
                             "resampler is not part of it; wire.convert_live_pcm16 takes raw samples at any rate"
                             % (int(in_sr), self.model_sr))
        if dtype not in (torch.float32, torch.int16):
            raise TypeError("convert_live: dtype must be int16 or float32, got %s" % dtype)
        from .models import _host_sid
        sids = []
        for name, sid in (("sid_src", _host_sid(sid_src)), ("sid_tgt", _host_sid(sid_tgt))):
            if torch.is_tensor(sid):
                if sid.numel() != 1:
                    raise ValueError("convert_live: %s must be one speaker id" % name)
                sid = sid.reshape(()).item()
            if isinstance(sid, bool) or int(sid) != sid:
                raise TypeError("convert_live: %s must be an integer" % name)
            sids.append(int(sid))
        self.sid_src, self.sid_tgt = sids
        self.noise_scale = float(noise_scale)
        if not math.isfinite(self.noise_scale) or self.noise_scale < 0:
            raise ValueError("convert_live: noise_scale must be finite and >= 0")
        self.n_fft = net._check_conversion("convert_live", self.hop_size, self.win_size)
        net._check_speakers(self.sid_src, self.sid_tgt)
        self.max_samples = int(max_samples)
        self.max_frames = int(_capi.lib().mbv_spectrogram_frames(max(self.max_samples, 0), self.n_fft, self.hop_size))
        if self.max_samples < 1 or self.max_frames < 1:
            raise ValueError("convert_live: max_samples %d gives no spectrogram frame (n_fft %d, hop_size %d)"
                             % (self.max_samples, self.n_fft, self.hop_size))
        h = net._handle_not_bf16("convert_live", "convert with voice_conversion", why="")
        cfg = net._config_struct()
        self._plan = LivePlan(self.n_fft, self.hop_size, converter_context(cfg)[1], decoder_context(cfg)[1],
                              chunk_frames, max_chunk_frames, convert_frames, ahead=ahead, model_sr=self.model_sr,
                              samples_per_frame=net.cfg.samples_per_frame)
        self.ahead, self.seam = ahead, self._plan.seam
        self._cfg_struct = cfg
        self.chunk_frames, self.max_chunk_frames = int(chunk_frames), int(max_chunk_frames)
        self._net, self._h = net, h
        dev = net._device()
        I, F = net.cfg.inter_channels, self.max_frames
        self.spf = net.cfg.samples_per_frame
        self.dtype = dtype
        with torch.cuda.device(dev), torch.no_grad():
            if seed is not None:
                # the capacity buffer, once, as one block: element (c, t) does not depend on F
                self.noise = net.randn(seed, I, F, purpose=_capi.NOISE_POSTERIOR).unsqueeze(0)
            elif noise is None:
                self.noise = torch.randn(1, I, F, device=dev, dtype=torch.float32)
            else:
                if not torch.is_tensor(noise) or noise.dtype != torch.float32 or tuple(noise.shape) != (1, I, F):
                    raise ValueError("convert_live: noise must be a float32 tensor [1, %d, %d] (inter_channels, the frames "
                                     "of max_samples)" % (I, F))
                self.noise = noise.to(dev).contiguous()
            self.samples = torch.zeros(self.max_samples, device=dev, dtype=dtype)
            self.z = torch.zeros(1, I, F, device=dev, dtype=torch.float32)
            self.o = torch.empty(1, 1, self.spf * F, device=dev, dtype=torch.float32)
            self.g = net.emb_g(torch.tensor([self.sid_tgt], dtype=torch.int64, device=dev))
            # what the previous decode gave for the head of the next chunk (`Ahead(seam_ms=)`); never handed out
            self._stash = torch.zeros(self.seam, device=dev, dtype=torch.float32) if self.seam else None
        self._stashed = 0             # samples of the stash that hold an overhang
        self.y_lengths = None
        self._chunks = []             # (first, count) of every chunk decoded so far, in order
        self._next = 0                # the chunk poll() hands out next
        self._decoded = 0             # == len(_chunks)
        # the ids go to the converter on every tick: a voice among them stays defined until the stream has finished
        net._hold_voices(self, self.sid_src, self.sid_tgt)

    def __repr__(self):
        return "LiveStream(sid %d -> %d, %d of %d samples%s)" % (self.sid_src, self.sid_tgt, self._plan.arrived,
                                                                 self.max_samples, ", closed" if self._plan.closed else "")

    # ---- the recording
    @property
    def arrived(self):
        return self._plan.arrived

    @property
    def closed(self):
        return self._plan.closed

    @property
    def frames(self):
        """T, once closed (None before)."""
        return self._plan.total

    @property
    def z_frames(self):
        """z_hat frames converted so far: z[:, :, :z_frames] is final."""
        return self._plan.z_done

    def pending(self):
        """The z_hat range (a, b) the next `poll()` / `StreamPool.step()` converts, or None; with `ahead`, the list of
        the grid blocks it converts."""
        return self._plan.convert_due()

    @property
    def schedule(self):
        """`chunk_schedule(T, ...)` once closed; before, the chunks decoded so far (a prefix of it)."""
        if self._plan.closed:
            return chunk_schedule(self._plan.total, self.chunk_frames, self.max_chunk_frames)
        return list(self._chunks)

    @property
    def finished(self):
        return self._plan.all_released and self._next >= self._decoded

    def push(self, samples):
        if not torch.is_tensor(samples):
            raise TypeError("push takes a 1-D tensor of %s samples" % self.dtype)
        if samples.dtype != self.dtype:
            raise TypeError("push: the stream was opened for %s samples, got %s" % (self.dtype, samples.dtype))
        if samples.dim() != 1:
            raise ValueError("push takes 1-D samples, got shape %s" % (tuple(samples.shape),))
        if self._plan.closed:
            raise ValueError("push after close()")
        n, a = samples.numel(), self._plan.arrived
        if a + n > self.max_samples:
            raise ValueError("push: %d + %d samples exceed the stream's capacity of %d (max_samples)" % (a, n, self.max_samples))
        if n:
            self.samples[a:a + n].copy_(samples)
            self._plan.push(n)

    def close(self):
        if self._plan.closed:
            return
        check_closable(self._plan.arrived, self.model_sr, self.n_fft, self.hop_size)
        self._plan.close()

    # ---- for an owner that fills `samples` itself (wire.LiveWire resamples into it)
    @property
    def plan(self):
        """The stream's `LivePlan` (integers only)."""
        return self._plan

    @property
    def chunks(self):
        """(first, count) of every chunk decoded so far, in order (by `poll` or by a pool)."""
        return tuple(self._chunks)

    @property
    def all_decoded(self):
        """The recording is closed and its last chunk is decoded."""
        return self._plan.all_released

    def fed(self, count, last=False):
        """The owner wrote `count` more samples behind `arrived` into `samples` (no copy here); `last` closes the
        recording, through `close()` and its check."""
        if count:
            self._plan.push(count)
        if last:
            self.close()

    def check_handle(self):
        self._check_handle()

    # ---- what a pool shares (StreamPool.step); poll() is the stand-alone form of the same steps
    def _check_handle(self):
        if self._net._handle is not self._h:
            raise RuntimeError("the model's handle was re-created (device move) since this stream started")

    def _window_frames(self, a, b):
        out, L, p = (C.c_int32 * 2)(), _capi.lib(), self._plan
        if p.ahead is None:
            rc = L.mbv_convert_window(C.byref(self._cfg_struct), a, b - a, p.spec_final, C.byref(out))
        else:
            rc = L.mbv_convert_window_ahead(C.byref(self._cfg_struct), a, b - a, p.ahead.conv, p.spec_final, C.byref(out))
        if rc:
            raise _capi.MbvError("mbv_convert_window refused [%d, %d)" % (a, b))
        return int(out[1]) - int(out[0])

    def _fill_range(self, row, a, b):
        row.wave, row.arrived, row.closed = self.samples.data_ptr(), self._plan.arrived, int(self._plan.closed)
        row.wave_dtype = _capi.WAVE_PCM16 if self.dtype == torch.int16 else _capi.WAVE_F32
        row.sid_src, row.sid_tgt, row.first, row.count = self.sid_src, self.sid_tgt, a, b - a
        row.noise, row.noise_stride, row.noise_scale = self.noise.data_ptr(), self.noise.stride(1), self.noise_scale
        row.z, row.z_stride = self.z.data_ptr(), self.z.stride(1)

    def _fill_chunk(self, k, first, count):
        """-> the route length: the class a finished recording of more than 256 frames is decoded in."""
        t = self._plan.t_frames(first, count)      # (what is converted; with `ahead` the chunk's canonical D)
        k.z, k.z_stride, k.t_frames = self.z.data_ptr(), self.z.stride(1), t
        k.g, k.first, k.o = self.g.data_ptr(), first, self.o.data_ptr()
        k.count = count + self._plan.overhang(first, count)
        return max(t, 257)

    def _fill_seam(self, row, first, count):
        """The `MbvSeamRow` of chunk (first, count), just decoded with its overhang: its head is blended with the stash,
        then its overhang is stashed.  -> whether the row does anything."""
        spf, S = self.spf, self.seam
        head = min(self._stashed, S, spf * count)
        over = min(S, spf * self._plan.overhang(first, count))
        row.o, row.o_samples, row.stash, row.seam = self.o.data_ptr(), self.o.shape[-1], self._stash.data_ptr(), S
        row.head_first, row.head_count = spf * first, head
        row.over_first, row.over_count = spf * (first + count), over
        self._stashed = over
        return bool(head or over)

    def _due_blocks(self):
        return self._plan.due_blocks()

    def _next_chunk(self):
        return self._plan.next_chunk()

    def _chunk_decoded(self, first, count):
        self._plan.released(first, count)
        self._chunks.append((first, count))
        self._decoded += 1

    def _drained(self):
        return self._plan.all_released

    def _convert(self):
        if self._plan.ahead is not None:           # the grid blocks due, as rows of the planner's runs
            _convert_live(self._net, [self])
            return
        due = self._plan.convert_due()
        if due is None:
            return
        self._check_handle()
        _convert_ranges(self._net, [(self, due)], self.hop_size, self.win_size)

    def poll(self):
        """Convert what the rules allow, decode every chunk that has become decodable (all of them in one
        `mbv_decode_chunks_routed` call; under a seam one call and one `mbv_seam_rows` launch per chunk) and hand out
        every chunk not handed out yet: [(first_sample, view), ...]."""
        self._convert()
        todo = self._plan.decodable()
        if todo:
            self._check_handle()
            # under a seam a chunk's overhang lies where the next chunk is decoded, and is stashed in between: a call each
            for part in ([[c] for c in todo] if self.seam else [todo]):
                _decode_chunks(self._net, [(self, first, count) for first, count in part])
        out = []
        while self._next < self._decoded:
            first, count = self._chunks[self._next]
            out.append((self.spf * first, self.o[:, :, self.spf * first:self.spf * (first + count)]))
            self._next += 1
        if self._plan.all_released and self.y_lengths is None:
            self.y_lengths = torch.full((1,), self._plan.total, dtype=torch.int64, device=self.z.device)
        return out

    def result(self):
        """o[:, :, :256 T] of the finished stream."""
        if not self.finished:
            raise RuntimeError("result(): the stream is not finished (close() it and poll() until `finished`)")
        return self.o[:, :, :self.spf * self._plan.total]


class DecodeStream:
    """Iterator over (first_sample, o[:, :, a:b]) of one decode, one `mbv_decode_range` launch per chunk.

    `o` [B, 1, spf T'] is allocated once, before the first chunk; chunk i is decoded when the iterator reaches it,
    on the caller's current stream at that moment, and its view is ordered on that stream like every other output.
    All state lives in tensors the stream owns (z, g, o), so a paused stream survives other calls on the same model
    (`infer`, `dec`, another stream).  `y_lengths` is set by `infer_stream`.

    A `StreamPool` may decode chunks ahead of the iterator (`_decoded` > `_next`): `next()` then hands such a chunk out
    without launching anything, and decodes alone otherwise — the same bytes either way."""

    def __init__(self, net, handle, z, g, chunk_frames, max_chunk_frames):
        self._net, self._h = net, handle
        self.z, self.g = z, g
        B, _, Tp = z.shape
        self.spf = net.cfg.samples_per_frame
        self.schedule = chunk_schedule(Tp, chunk_frames, max_chunk_frames)
        self.o = torch.empty(B, 1, self.spf * Tp, device=z.device, dtype=torch.float32)
        self.y_lengths = None
        self.marks = None             # token marks in z-frames (`infer_stream(marks=True)`); a converted stream has none
        self.fit_scale = self.fit_status = None     # the factor and status of `fit_frames=`, else None
        self.frame_gain = None        # fp32 [B, F + 1] frame gains of `infer_stream(gain=)`, else None
        self.warp = None              # the `WarpMap` of `infer_stream(pitch=)`, else None
        self._next = 0                # the chunk next() hands out
        self._decoded = 0             # the first chunk not decoded yet (>= _next; ahead of it only through a pool)

    def __len__(self):
        return len(self.schedule)

    def __iter__(self):
        return self

    def __next__(self):
        if self._next >= len(self.schedule):
            raise StopIteration
        first, count = self.schedule[self._next]
        a, b = self.spf * first, self.spf * (first + count)
        if self._next < self._decoded:            # a pool decoded it already, on the stream current at its step
            self._next += 1
            return a, self.o[:, :, a:b]
        net, h = self._net, self._h
        if net._handle is not h:
            raise RuntimeError("the model's handle was re-created (device move) since this stream started")
        B, _, Tp = self.z.shape
        with torch.cuda.device(self.z.device):
            net._ensure_handle()                  # (re-uploads weights edited in place, as every entry does)
            net._launch(h, "mbv_decode_range", self.z, self.g, B, Tp, first, count, self.o, self.o.stride(0))
        self._next += 1
        self._decoded = self._next
        return a, self.o[:, :, a:b]

    def run(self):
        """Decode every remaining chunk; -> o."""
        for _ in self:
            pass
        return self.o

    # ---- what a pool shares (StreamPool.step), as `LiveStream` has it
    def _due_blocks(self):
        return []                     # z is whole

    def _next_chunk(self):
        return self.schedule[self._decoded] if self._decoded < len(self.schedule) else None

    def _fill_chunk(self, k, first, count):
        """-> None: a finished utterance is decoded in the class of its own length."""
        k.z, k.z_stride, k.t_frames = self.z.data_ptr(), self.z.stride(1), self.z.shape[2]
        k.g = self.g.data_ptr() if self.g is not None else None
        k.first, k.count, k.o = first, count, self.o.data_ptr()

    def _chunk_decoded(self, first, count):
        self._decoded += 1

    def _drained(self):
        return self._decoded >= len(self.schedule)

    def _truncate(self, n_chunks):
        """A revoked stream (`wire.PcmStream.revoke`) decodes its first `n_chunks` chunks only: the later ones are
        never issued (n_chunks >= the chunks decoded so far)."""
        self.schedule = self.schedule[:max(int(n_chunks), self._decoded)]


class StreamPool:
    """The next chunk of many `DecodeStream`s of one model in one `mbv_decode_chunks` call per `step()`.

    The pool only shares launches; it does not schedule.  `step()` decodes the next not yet decoded chunk of every
    pooled stream that has one (or of those named) and returns `[(st, first_sample, view), ...]`; the chunks count as
    decoded ahead on their streams, so `next(st)` — and a `wire.PcmStream` over `st` — afterwards hands them out
    without a launch.  A stream may be advanced through the pool, alone, or both in turn.  Streams may be added at
    any time, one by one (`add`) or as the requests they come from (`admit`); finished ones drop out, and `remove`
    drops one that is not (a revoked request).

    A `LiveStream` is a member like any other: `step()` first converts the pending windows of all live members in one
    `mbv_convert_ranges` run, then decodes at most one decodable chunk of each along with the others' chunks; a live
    member with nothing decodable yet is skipped and stays, and its next `poll()` hands the pooled chunks out."""

    def __init__(self, net):
        self._net = net
        self.streams = []

    def __len__(self):
        return len(self.streams)

    def add(self, st):
        if not isinstance(st, (DecodeStream, LiveStream)):
            raise TypeError("StreamPool.add takes a DecodeStream (net.dec_stream / net.infer_stream) or a LiveStream "
                            "(net.convert_live)")
        if st.z.shape[0] != 1:
            raise ValueError("StreamPool takes streams of ONE utterance (this one has %d rows): a pooled chunk is bitwise "
                             "its utterance's stand-alone decode, and a row of a batch is measured against the batch's "
                             "one-shot decode, a different yardstick (decode it with lengths= instead)" % st.z.shape[0])
        if st._net is not self._net:
            raise ValueError("the stream belongs to another model")
        if st.z.device != self._net._device():
            raise ValueError("the stream lives on %s, the pool's model on %s" % (st.z.device, self._net._device()))
        if not any(st is m for m in self.streams):
            self.streams.append(st)
        return st

    def remove(self, st):
        """Drops a member (a revoked request, in a pool without a wire): none of its later chunks is decoded by this
        pool.  ValueError for a stream that is not a member."""
        if not any(st is m for m in self.streams):
            raise ValueError("StreamPool.remove names a stream that is not in the pool")
        self.streams = [m for m in self.streams if m is not st]

    def admit(self, requests):
        """`net.infer_streams(requests)` + `add`: the front half of a tick's new requests in one padded run per class
        of `net.admit_plan` and one host read-back; -> their streams, in order.  A list that is all
        `models.ConvertRequest` goes through `net.convert_streams` instead (audio requests); a list that
        mixes the two kinds is a TypeError.  All or nothing: when a request is refused or flagged, the exception
        passes through, no stream is created and the pool is unchanged."""
        from .models import ConvertRequest
        reqs = list(requests)
        n_audio = sum(isinstance(r, ConvertRequest) for r in reqs)
        if n_audio and n_audio != len(reqs):
            raise TypeError("admit takes a list that is all models.Request or all models.ConvertRequest "
                            "(%d of %d items are ConvertRequest): admit the two kinds in two calls" % (n_audio, len(reqs)))
        sts = self._net.convert_streams(reqs) if n_audio else self._net.infer_streams(reqs)
        for st in sts:
            self.add(st)
        return sts

    def _convert_live(self, members):
        """The pending z_hat windows of every live member, bounded or not, in one `mbv_convert_ranges` run per run of
        the planner."""
        _convert_live(self._net, members)

    def step(self, streams=None):
        """Live members first convert their pending windows together (`_convert_live`); then at most one chunk per
        member is decoded in the one call.  A live member with nothing decodable is skipped and stays pooled."""
        if streams is None:
            members = list(self.streams)
        else:
            members = list(streams)
            for st in members:
                if not any(st is m for m in self.streams):
                    raise ValueError("step(streams=...) names a stream that is not in the pool")
        self.streams = [st for st in self.streams if not st._drained()]
        members = [st for st in members if not st._drained()]
        if not members:
            return []
        net = self._net
        self._convert_live(members)
        work = []                     # (stream, first, count)
        for st in members:
            if net._handle is not st._h:
                raise RuntimeError("the model's handle was re-created (device move) since a pooled stream started")
            nxt = st._next_chunk()
            if nxt is not None:
                work.append((st,) + nxt)
        if not work:
            return []
        _decode_chunks(net, work)
        self.streams = [st for st in self.streams if not st._drained()]
        return [(st, st.spf * first, st.o[:, :, st.spf * first:st.spf * (first + count)]) for st, first, count in work]
