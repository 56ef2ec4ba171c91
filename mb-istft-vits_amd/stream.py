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

Text that is still arriving: a `TextStream` (`net.infer_live`) is ONE utterance whose tokens are pushed as a language
model produces them.  Blocks of tokens are encoded from text prefixes (`TextPlan`, `TextAhead`), length-regulated into
the stream's own z_p at a running frame offset, the reverse flows run on windows of it, and the decode side is the
live stream's; the audio is a pure function of the token sequence, whatever the pushes.
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


def _decode_and_hand_out(st):
    """The back half of `LiveStream.poll` and `TextStream.poll`: decode every chunk of `st` that has become decodable,
    hand out every chunk not handed out yet as [(first_sample, view), ...], and set `y_lengths` once all are released."""
    todo = st._plan.decodable()
    if todo:
        st._check_handle()
        # under a seam a chunk's overhang lies where the next chunk is decoded, and is stashed in between: a call each
        for part in ([[c] for c in todo] if st.seam else [todo]):
            _decode_chunks(st._net, [(st, first, count) for first, count in part])
    out = []
    while st._next < st._decoded:
        first, count = st._chunks[st._next]
        out.append((st.spf * first, st.o[:, :, st.spf * first:st.spf * (first + count)]))
        st._next += 1
    if st._plan.all_released and st.y_lengths is None:
        st.y_lengths = torch.full((1,), st._plan.total, dtype=torch.int64, device=st.z.device)
    return out


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


def _seam_frames(seam_samples, dec, chunk_frames, seam_ms, model_sr, samples_per_frame):
    """The overhang, in frames, of a seam of `seam_samples` (ceil(S / spf)); ValueError unless 1 <= S <= the samples of
    the `dec` frames a chunk looks ahead and of the smallest chunk."""
    S, spf = int(seam_samples), int(samples_per_frame)
    if not 1 <= S <= spf * min(dec, chunk_frames):
        raise ValueError("a seam of %g ms is %d samples at %d Hz: it must be 1 .. %d, the samples of the dec = %d "
                         "frames a chunk looks ahead and of the smallest chunk (%d frames)"
                         % (seam_ms, S, int(model_sr), spf * min(dec, chunk_frames), dec, chunk_frames))
    return -(-S // spf)


class ChunkPlan:
    """Which chunks of a z that is still growing may be decoded, and from what: the rules `LivePlan` (z_hat converted
    from a recording) and `TextPlan` (z flowed from a text) share.  z frames [0, `z_done`) exist (`advanced`); T is the
    utterance's length once it is known, None before.

      dec None   chunk (first, count) is decodable iff z frames up to first + count + r_dec exist, or T is known and all
                 of [0, T) do; it is decoded from what exists (`t_frames` = z_done)
      dec = d    it is decoded with t_frames = D = min(first + count + d, T), decodable iff z frames up to D exist, and
                 `overhang` = min(over_frames, D - first - count) frames past its end for a seam
    Chunks are those of `chunk_schedule(T, chunk_frames, max_chunk_frames)`: only the cut of the last one depends on T."""

    def __init__(self, r_dec, chunk_frames, max_chunk_frames, dec=None, over_frames=0):
        c, cap = int(chunk_frames), int(max_chunk_frames)
        if c < 1 or cap < c:
            raise ValueError("need 1 <= chunk_frames <= max_chunk_frames (got %d, %d)" % (c, cap))
        self.r_dec, self.dec, self.over_frames = int(r_dec), dec, int(over_frames)
        self.z_done = 0
        self.first, self.c, self.cap, self.c0 = 0, c, cap, c     # the next chunk to release

    def advanced(self, a, b):
        if a != self.z_done or b <= a:
            raise ValueError("ranges are converted in order, once")
        self.z_done = b

    def decodable(self, T):
        first, c, out = self.first, self.c, []
        while True:
            if self.dec is not None:           # z up to the chunk's D (of the uncut chunk while T is not known)
                if T is not None and first >= T:
                    break
                n = min(c, T - first) if T is not None else c
                if self.z_done < self.t_frames(first, n, T):
                    break
            elif T is not None:
                if self.z_done < T or first >= T:
                    break
                n = min(c, T - first)
            else:
                if self.z_done < first + c + self.r_dec:
                    break
                n = c
            out.append((first, n))
            first, c = first + n, min(2 * c, self.cap)
        return out

    def t_frames(self, first, count, T):
        if self.dec is None:
            return self.z_done
        D = first + count + self.dec
        return min(D, T) if T is not None else D

    def overhang(self, first, count, T):
        return min(self.over_frames, self.t_frames(first, count, T) - first - count) if self.over_frames else 0

    def released(self, first, count):
        if first != self.first:
            raise ValueError("chunks are released in order")
        self.first += count
        self.c = min(2 * self.c, self.cap)

    def all_released(self, T):
        return T is not None and self.first >= T


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
        self.ahead, self.seam, over = ahead, 0, 0
        if ahead is not None:
            if not isinstance(ahead, Ahead):
                raise TypeError("ahead must be a stream.Ahead or None, got %r" % (ahead,))
            if ahead.conv > self.r_conv or ahead.dec > self.r_dec:
                raise ValueError("%r looks further than the model can: conv <= %d, dec <= %d" % (ahead, self.r_conv, self.r_dec))
            if ahead.seam_ms:
                if model_sr is None or samples_per_frame is None:
                    raise ValueError("a seam needs model_sr and samples_per_frame")
                self.seam = ahead.seam_samples(model_sr)
                over = _seam_frames(self.seam, ahead.dec, c, ahead.seam_ms, model_sr, samples_per_frame)
        self.arrived, self.closed = 0, False
        self._chunks = ChunkPlan(r_dec, c, cap, None if ahead is None else ahead.dec, over)

    @property
    def z_done(self):
        """z_hat frames [0, z_done) are converted."""
        return self._chunks.z_done

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
        self._chunks.advanced(a, b)

    def decodable(self):
        """[(first, count), ...]: the chunks not released yet that are decodable now, in order (`ChunkPlan`)."""
        return self._chunks.decodable(self.total)

    def t_frames(self, first, count):
        """D of chunk (first, count): the z_hat frames [0, D) it is decoded from, min(first + count + dec, T) (T once
        closed; a chunk decodable before lies wholly inside the recording).  Without `ahead`: what is converted."""
        return self._chunks.t_frames(first, count, self.total)

    def overhang(self, first, count):
        """Frames chunk (first, count) is decoded past its end for the seam (0 without one)."""
        return self._chunks.overhang(first, count, self.total)

    def lag(self):
        """(arrived, frames): the sample count at which the first chunk is released when `poll()` follows every push
        however small, and the steady-state lag: the largest distance, over the chunks of full size, from a chunk's
        first frame to the number of final spectrogram frames its release waits for.  Pure integers; without `ahead`
        the same arithmetic at (R_conv, R_dec), which the unbounded stream meets under such pushes."""
        cf, conv, dec = self.convert_frames, self.conv_ahead, self.dec_ahead
        need = lambda first, c: -(-(first + c + dec) // cf) * cf + conv     # final frames chunk (first, c) waits for
        first, c, cap = 0, self._chunks.c0, self._chunks.cap
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
        self._chunks.released(first, count)

    @property
    def all_released(self):
        return self._chunks.all_released(self.total)


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
        return _decode_and_hand_out(self)

    def result(self):
        """o[:, :, :256 T] of the finished stream."""
        if not self.finished:
            raise RuntimeError("result(): the stream is not finished (close() it and poll() until `finished`)")
        return self.o[:, :, :self.spf * self._plan.total]


def text_context(config_struct):
    """(R, R) of `mbv_text_context` for an `_capi.MbvConfig` (host only): z frame t depends on z_p frames
    [t - R, t + R] only."""
    out = (C.c_int32 * 2)()
    if _capi.lib().mbv_text_context(C.byref(config_struct), C.byref(out)):
        raise _capi.MbvError("mbv_text_context failed")
    return int(out[0]), int(out[1])


class TextAhead:
    """How far a live text looks ahead.  `tokens` = A: token block k is encoded from the text prefix of
    min((k + 1) block_tokens + A, N) tokens; None = the whole text (every block waits for `close()`).  `dec`: None =
    the decoder's full reach (the rules of `LivePlan` without `ahead`), an integer 0 <= dec <= R_dec the canonical
    t_frames of `Ahead(., dec, seam_ms)`; `seam_ms` (needs `dec`) as `Ahead` takes it.  With bounded `tokens` the
    stream is an approximation with an exact definition: how far a trained text encoder looks ahead is a property of
    its weights."""

    __slots__ = ("tokens", "dec", "seam_ms")

    def __init__(self, tokens=None, dec=None, seam_ms=0.0):
        for name, v in (("tokens", tokens), ("dec", dec)):
            if v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError("TextAhead: %s must be an integer or None, got %r" % (name, v))
            if v < 0:
                raise ValueError("TextAhead: %s must be >= 0, got %d" % (name, v))
        if isinstance(seam_ms, bool) or not isinstance(seam_ms, (int, float, np.integer, np.floating)):
            raise TypeError("TextAhead: seam_ms must be a number of milliseconds, got %r" % (seam_ms,))
        if not math.isfinite(seam_ms) or seam_ms < 0:
            raise ValueError("TextAhead: seam_ms must be finite and >= 0, got %r" % (seam_ms,))
        if seam_ms and dec is None:
            raise ValueError("TextAhead: a seam needs a bounded dec (with the full reach the chunks meet as they are)")
        self.tokens = None if tokens is None else int(tokens)
        self.dec = None if dec is None else int(dec)
        self.seam_ms = float(seam_ms)

    def __repr__(self):
        return "TextAhead(tokens=%r, dec=%r%s)" % (self.tokens, self.dec,
                                                   ", seam_ms=%g" % self.seam_ms if self.seam_ms else "")


class TextPlan:
    """What a text that is still arriving may encode, flow and decode, in pure integers (no tensor, no GPU); bt =
    `block_tokens`, A = `ahead.tokens`, R = `r_flow`, N the tokens once closed.

      token block k         tokens [k bt, min((k + 1) bt, N)), encoded from the prefix of E_k = min((k + 1) bt + A, N)
                            tokens (A None: E_k = N); due iff E_k tokens have arrived, or closed.  `due_blocks()` ->
                            [(k, E_k), ...] in order; `encoded(k, frames)` takes the block's durations as read back
      frames                F_t = the sum of the durations in front of token t (`marks`), P those of the encoded blocks
      z frames [0, b)       may be flowed with b = P once closed and every block is encoded (`complete`), else
                            b = max(0, P - R); `flow_due()` -> (a, b) when >= `flow_frames` new frames may be, or at
                            the end; `flowed(a, b)`
      chunk (first, count)  `LivePlan`'s rules on the flowed frames: without `ahead.dec` decodable iff z frames up to
                            first + count + R_dec are flowed (or complete), decoded from what is flowed; with it,
                            decoded with t_frames = min(first + count + dec, T), overhang and seam as `Ahead` has them
    so that what is encoded, flowed and decoded, and from what, does not depend on the pushes."""

    def __init__(self, block_tokens, r_flow, r_dec, chunk_frames=32, max_chunk_frames=256, flow_frames=32, ahead=None,
                 model_sr=None, samples_per_frame=None):
        bt, ff = int(block_tokens), int(flow_frames)
        if bt < 1:
            raise ValueError("block_tokens must be >= 1")
        if ff < 1:
            raise ValueError("flow_frames must be >= 1")
        if int(r_flow) < 0 or int(r_dec) < 0:
            raise ValueError("r_flow and r_dec must be >= 0")
        if ahead is None:
            ahead = TextAhead()
        if not isinstance(ahead, TextAhead):
            raise TypeError("ahead must be a stream.TextAhead or None, got %r" % (ahead,))
        if ahead.dec is not None and ahead.dec > int(r_dec):
            raise ValueError("%r looks further than the decoder can: dec <= %d" % (ahead, int(r_dec)))
        self.block_tokens, self.r_flow, self.flow_frames, self.ahead = bt, int(r_flow), ff, ahead
        self._chunks = ChunkPlan(r_dec, chunk_frames, max_chunk_frames, ahead.dec)
        self.seam = 0
        if ahead.seam_ms:
            if model_sr is None or samples_per_frame is None:
                raise ValueError("a seam needs model_sr and samples_per_frame")
            self.seam = int(round(ahead.seam_ms * int(model_sr) / 1000.0))
            self._chunks.over_frames = _seam_frames(self.seam, ahead.dec, self._chunks.c0, ahead.seam_ms, model_sr,
                                                    samples_per_frame)
        self.arrived, self.closed = 0, False
        self.blocks = 0                        # token blocks [0, blocks) are encoded
        self.durations = []                    # frames of every encoded token
        self.marks = [0]                       # F_t of every encoded token, then P

    def push(self, n):
        if self.closed:
            raise ValueError("push after close()")
        if int(n) < 0:
            raise ValueError("push: a negative count")
        self.arrived += int(n)

    def close(self):
        if not self.closed and self.arrived < 1:
            raise ValueError("close(): the text is empty")
        self.closed = True

    @property
    def frames(self):
        """P: the frames of the encoded blocks."""
        return self.marks[-1]

    @property
    def complete(self):
        """Closed, and every block is encoded: P is the utterance's T."""
        return self.closed and self.blocks * self.block_tokens >= self.arrived

    @property
    def total(self):
        """T, once complete (None before)."""
        return self.frames if self.complete else None

    @property
    def z_done(self):
        """z frames [0, z_done) are flowed."""
        return self._chunks.z_done

    def due_blocks(self):
        """[(k, E_k), ...]: every token block to encode now, in order."""
        bt, A, out, k = self.block_tokens, self.ahead.tokens, [], self.blocks
        while True:
            if self.closed:
                if k * bt >= self.arrived:
                    break
                E = self.arrived if A is None else min((k + 1) * bt + A, self.arrived)
            else:
                if A is None or (k + 1) * bt + A > self.arrived:
                    break
                E = (k + 1) * bt + A
            out.append((k, E))
            k += 1
        return out

    def block_tokens_of(self, k, E):
        """The token range [a, b) of block k encoded from a prefix of E tokens."""
        return k * self.block_tokens, min((k + 1) * self.block_tokens, E)

    def encoded(self, k, frames):
        frames = [int(v) for v in frames]
        if k != self.blocks:
            raise ValueError("blocks are encoded in order, once")
        if not frames or len(frames) > self.block_tokens or min(frames) < 0:
            raise ValueError("block %d: 1 .. %d durations >= 0 expected" % (k, self.block_tokens))
        if len(self.durations) + len(frames) > self.arrived:
            raise ValueError("block %d: more durations than tokens have arrived" % k)
        for v in frames:
            self.durations.append(v)
            self.marks.append(self.marks[-1] + v)
        self.blocks += 1

    def flow_due(self):
        """The z range [a, b) to flow now, or None."""
        P = self.frames
        b = P if self.complete else max(0, P - self.r_flow)
        a = self._chunks.z_done
        if b > a and (self.complete or b - a >= self.flow_frames):
            return a, b
        return None

    def flowed(self, a, b):
        self._chunks.advanced(a, b)

    def decodable(self):
        """[(first, count), ...]: the chunks not released yet that are decodable now, in order (`ChunkPlan`)."""
        return self._chunks.decodable(self.total)

    def next_chunk(self):
        d = self.decodable()
        return d[0] if d else None

    def t_frames(self, first, count):
        return self._chunks.t_frames(first, count, self.total)

    def overhang(self, first, count):
        return self._chunks.overhang(first, count, self.total)

    def released(self, first, count):
        self._chunks.released(first, count)

    @property
    def all_released(self):
        return self._chunks.all_released(self.total)


def _text_tick(net, members):
    """The front half of one tick for the text streams `members`: ONE `mbv_encode_rows` run per class of
    `mbv_admit_plan` over all due token blocks (one row is one prefix), one `mbv_take_tokens_rows` launch per run, ONE
    host read-back (the blocks' durations, -1 = the prefix was flagged), one `mbv_expand_ranges` launch, then the flow
    runs `mbv_flow_ranges_plan` cuts.  Nothing due: nothing is launched.  -> whether a member failed in this tick."""
    members = [st for st in members if not st.failed]
    due = [(st, k, E) for st in members for k, E in st._plan.due_blocks()]
    failed = False
    L = _capi.lib()
    if due:
        for st, _, _ in due:
            st._check_handle()
        h, dev, cfg = net._ensure_handle(), net._device(), net.cfg
        n_runs, run_of = net.admit_plan([E for _, _, E in due], splitk=L.mbv_get_option(h, b"splitk") != 0)
        if n_runs > 64:
            raise ValueError("a tick of %d encoder runs: at most 64 (the slots of mbv_encode_rows)" % n_runs)
        runs = [[i for i in range(len(due)) if run_of[i] == r] for r in range(n_runs)]
        ranges = [st._plan.block_tokens_of(k, E) for st, k, E in due]
        with torch.cuda.device(dev), torch.no_grad():
            hip_stream = net._stream(dev)
            # ids (zero-padded to the run's longest prefix), lengths and sids of every run: ONE host tensor, one copy
            parts = []
            for m in runs:
                T = max(due[i][2] for i in m)
                for i in m:
                    st, _, E = due[i]
                    parts.append(st._ids[:E] + [0] * (T - E))
                parts.append([due[i][2] for i in m])
                if net.n_speakers > 0:
                    parts.append([due[i][0].sid for i in m])
            packed = torch.tensor([v for p in parts for v in p], dtype=torch.int64).to(dev)
            noise_w = [None] * len(due)
            if cfg.use_sdp:                        # the first E columns of both rows of every stream's own draw
                flat_w = torch.cat([st.noise_w[:, :E].reshape(-1) for st, _, E in due])
                o = 0
                for i, (_, _, E) in enumerate(due):
                    noise_w[i] = flat_w.data_ptr() + 4 * o
                    o += 2 * E
            y_buf = torch.empty(len(due), dtype=torch.int64, device=dev)
            dur_buf = torch.empty(sum(b - a for a, b in ranges), dtype=torch.int32, device=dev)
            at, o = [], 0
            for a, b in ranges:
                at.append(o)
                o += b - a
            o, row0 = 0, 0
            for r, m in enumerate(runs):
                B, T = len(m), max(due[i][2] for i in m)
                ids, lens = packed.data_ptr() + 8 * o, packed.data_ptr() + 8 * (o + B * T)
                sid = packed[o + B * T + B:o + B * T + 2 * B] if net.n_speakers > 0 else None
                o += B * T + (2 * B if net.n_speakers > 0 else B)
                rows = (_capi.MbvEncRow * B)()
                take = (_capi.MbvTakeRow * B)()
                for j, i in enumerate(m):
                    st, k, E = due[i]
                    rows[j].length_scale, rows[j].noise_scale_w = st.length_scale, st.noise_scale_w
                    rows[j].noise_w, rows[j].t_text = noise_w[i], E
                    t = take[j]
                    t.src, (t.a, t.b) = j, ranges[i]
                    t.y_length = y_buf.data_ptr() + 8 * (row0 + j)
                    t.stats, t.dur, t.stride = st.stats.data_ptr(), st.dur.data_ptr(), st.max_tokens
                    t.dur_copy = dur_buf.data_ptr() + 4 * at[i]
                net._launch(h, "mbv_encode_rows", r, C.c_void_p(ids), C.c_void_p(lens), sid, B, T, rows,
                            C.c_void_p(y_buf.data_ptr() + 8 * row0), stream=hip_stream)
                net._launch(h, "mbv_take_tokens_rows", r, take, B, stream=hip_stream)
                row0 += B
            host = dur_buf.tolist()                # the one host sync of the tick
            expand, keep = [], []
            for i, (st, k, E) in enumerate(due):
                if st.failed:                      # an earlier block of this tick failed it
                    continue
                (a, b), d = ranges[i], host[at[i]:at[i] + ranges[i][1] - ranges[i][0]]
                if min(d) < 0:
                    st._fail(IndexError("infer_live: token block %d (tokens [%d, %d), encoded from %d tokens): index out of "
                                        "range in self (a token id or the sid outside the model's tables, or a duration "
                                        "outside the supported range)" % (k, a, b, E)))
                elif st._plan.frames + sum(d) > st.max_frames:
                    st._fail(ValueError("infer_live: token block %d (tokens [%d, %d)) ends at frame %d: beyond the stream's "
                                        "max_frames = %d" % (k, a, b, st._plan.frames + sum(d), st.max_frames)))
                else:
                    row = _capi.MbvExpandRange()
                    d_host = (C.c_int32 * len(d))(*d)
                    keep.append(d_host)
                    row.stats, row.dur, row.stride = st.stats.data_ptr(), st.dur.data_ptr(), st.max_tokens
                    row.dur_host, row.a, row.b = C.addressof(d_host), a, b
                    row.frame, row.max_frames = st._plan.frames, st.max_frames
                    row.noise, row.noise_stride, row.noise_scale = st.noise.data_ptr(), st.noise.stride(1), st.noise_scale
                    row.z_p, row.z_stride = st.z_p.data_ptr(), st.z_p.stride(1)
                    expand.append(row)
                    st._plan.encoded(k, d)
                    if st._plan.complete and st._plan.frames < 1:
                        st._fail(ValueError("infer_live: the text has no frames (every duration is 0)"))
                failed = failed or st.failed
            if expand:
                net._launch(h, "mbv_expand_ranges", (_capi.MbvExpandRange * len(expand))(*expand), len(expand),
                            stream=hip_stream)
    todo = [(st, st._plan.flow_due()) for st in members if not st.failed]
    todo = [(st, fd) for st, fd in todo if fd is not None]
    if todo:
        cfg_struct = todo[0][0]._cfg_struct
        n = len(todo)
        wl, out = (C.c_int32 * n)(), (C.c_int32 * 2)()
        for i, (st, (a, b)) in enumerate(todo):
            st._check_handle()
            if L.mbv_flow_window(C.byref(cfg_struct), a, b - a, st._plan.frames, C.byref(out)):
                raise _capi.MbvError("mbv_flow_window refused [%d, %d)" % (a, b))
            wl[i] = int(out[1]) - int(out[0])
        run_of = (C.c_int32 * n)()
        n_runs = L.mbv_flow_ranges_plan(C.byref(cfg_struct), n, wl, run_of)
        if n_runs < 1:
            raise ValueError("mbv_flow_ranges_plan refused the windows (one beyond the fused WN layers?)")
        for r in range(n_runs):
            part = [t for t, q in zip(todo, run_of) if q == r]
            rows = (_capi.MbvFlowRange * len(part))()
            for row, (st, (a, b)) in zip(rows, part):
                row.z_p, row.z_p_stride = st.z_p.data_ptr(), st.z_p.stride(1)
                row.P, row.complete, row.sid = st._plan.frames, int(st._plan.complete), st.sid or 0
                row.first, row.count, row.z, row.z_stride = a, b - a, st.z.data_ptr(), st.z.stride(1)
            net._call("mbv_flow_ranges", rows, len(part))
            for st, (a, b) in part:
                st._plan.flowed(a, b)
    return failed


class TextStream:
    """Synthesis of ONE utterance whose tokens are pushed as they arrive (`net.infer_live`): the text
    mirror of `LiveStream`.

    `push(ids)` appends tokens, `close()` ends the text, `poll()` runs one tick — the due token blocks through the text
    encoder and the duration predictor as prefixes, their columns into the stream's token tables, length regulation
    into the stream's own z_p, the reverse flows on the window that became computable, every chunk that became
    decodable — and returns `[(first_sample, view), ...]`.  The ids, the token tables, the noise, z_p, z, o and g
    belong to the stream, so other calls may run between any two polls.  The token statistics, the durations, z_p, z
    and every sample are a function of (ids, sid, scales, seed / noise, block_tokens, `TextAhead`, chunk schedule)
    only: not of the sizes of the pushes, of when `poll()` runs or of which streams share a `StreamPool`.  With
    `TextAhead(tokens=None)` a finished stream of more than 256 frames is bitwise `infer_stream` on the whole text with
    the same seed; bounded `tokens` is an approximation with an exact definition, and no claim about its quality is
    made.  Not part of a text stream: per-token `length_scale` / `extra_frames` / `fit_frames` / `gain` / `pitch`,
    `durations=`, `max_len`, a bounded flow look-ahead, and the wire layer (`PcmPool`, `stream_pcm16`)."""

    def __init__(self, net, sid=None, max_tokens=None, max_frames=None, noise_scale=1, length_scale=1, noise_scale_w=1.,
                 seed=None, noise=None, noise_w=None, block_tokens=16, ahead=None, chunk_frames=32, max_chunk_frames=256,
                 flow_frames=32, model_sr=None):
        from .models import _host_sid, _row_seeds
        if seed is not None:
            if noise is not None or noise_w is not None:
                raise ValueError("infer_live: seed= and noise= / noise_w= exclude each other")
            seed = _row_seeds(seed, 1, "infer_live: seed")[0][0]
        for name, v in (("max_tokens", max_tokens), ("max_frames", max_frames)):
            if v is None or isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError("infer_live: %s must be an integer >= 1 (the stream's buffers are allocated once)" % name)
        self.max_tokens, self.max_frames = int(max_tokens), int(max_frames)
        scales = []
        for name, v in (("noise_scale", noise_scale), ("length_scale", length_scale), ("noise_scale_w", noise_scale_w)):
            if torch.is_tensor(v) or isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise TypeError("infer_live: %s must be one number (per-token controls are not part of a text stream)" % name)
            if not math.isfinite(v) or v < 0:
                raise ValueError("infer_live: %s must be finite and >= 0" % name)
            scales.append(float(v))
        self.noise_scale, self.length_scale, self.noise_scale_w = scales
        sid = _host_sid(sid)
        if net.n_speakers > 0:
            if sid is None:
                raise ValueError("sid is required for a multi-speaker model (models.py:704-705)")
            if torch.is_tensor(sid):
                if sid.numel() != 1:
                    raise ValueError("infer_live: sid must be one speaker id")
                sid = sid.reshape(()).item()
            if isinstance(sid, bool) or int(sid) != sid:
                raise TypeError("infer_live: sid must be an integer")
            sid = int(sid)
            if not (0 <= sid < net.n_speakers or net._voice_defined(sid)):
                raise IndexError("index out of range in self (sid %d outside [0, %d))" % (sid, net.n_speakers))
        else:
            sid = None
        self.sid = sid
        h = net._handle_not_bf16("infer_live", "synthesise with infer_stream", why="")
        cfg = net._config_struct()
        self.spf = net.cfg.samples_per_frame
        self._plan = TextPlan(block_tokens, text_context(cfg)[1], decoder_context(cfg)[1], chunk_frames, max_chunk_frames,
                              flow_frames, ahead=ahead, model_sr=model_sr, samples_per_frame=self.spf)
        self.ahead, self.seam = self._plan.ahead, self._plan.seam
        self._cfg_struct = cfg
        self.chunk_frames, self.max_chunk_frames = int(chunk_frames), int(max_chunk_frames)
        self._net, self._h = net, h
        dev = net._device()
        I, F, N = net.cfg.inter_channels, self.max_frames, self.max_tokens
        with torch.cuda.device(dev), torch.no_grad():
            if seed is not None:
                # the capacity buffers, once, as one block each: element (c, t) does not depend on F / N
                self.noise = net.randn(seed, I, F, purpose=_capi.NOISE_PRIOR).unsqueeze(0)
            elif noise is None:
                self.noise = torch.randn(1, I, F, device=dev, dtype=torch.float32)
            else:
                if not torch.is_tensor(noise) or noise.dtype != torch.float32 or tuple(noise.shape) != (1, I, F):
                    raise ValueError("infer_live: noise must be a float32 tensor [1, %d, %d] (inter_channels, max_frames)"
                                     % (I, F))
                self.noise = noise.to(dev).contiguous()
            self.noise_w = None
            if net.cfg.use_sdp:
                if seed is not None:
                    self.noise_w = net.randn(seed, 2, N, purpose=_capi.NOISE_SDP)
                elif noise_w is None:
                    self.noise_w = torch.randn(2, N).to(dev)       # the CPU generator, as the reference's SDP draw
                else:
                    if not torch.is_tensor(noise_w) or noise_w.dtype != torch.float32 or tuple(noise_w.shape) != (2, N):
                        raise ValueError("infer_live: noise_w must be a float32 tensor [2, %d] (max_tokens)" % N)
                    self.noise_w = noise_w.to(dev).contiguous()
            self.stats = torch.zeros(2 * I, N, device=dev, dtype=torch.float32)      # m_p | logs_p of every token
            self.dur = torch.zeros(N, device=dev, dtype=torch.int32)
            self.z_p = torch.zeros(1, I, F, device=dev, dtype=torch.float32)
            self.z = torch.zeros(1, I, F, device=dev, dtype=torch.float32)
            self.o = torch.empty(1, 1, self.spf * F, device=dev, dtype=torch.float32)
            self.g = None
            if sid is not None:
                self.g = net._speaker_embedding(torch.tensor([sid], dtype=torch.int64, device=dev))
            self._stash = torch.zeros(self.seam, device=dev, dtype=torch.float32) if self.seam else None
        self._stashed = 0
        self._ids = []                # the tokens pushed so far, host ints
        self.y_lengths = None
        self._error = None
        self._chunks, self._next, self._decoded = [], 0, 0
        if sid is not None:
            net._hold_voices(self, sid)

    def __repr__(self):
        return "TextStream(%d of %d tokens%s, %d frames)" % (len(self._ids), self.max_tokens,
                                                             ", closed" if self._plan.closed else "", self._plan.frames)

    # ---- the text
    @property
    def tokens(self):
        """Tokens pushed so far."""
        return len(self._ids)

    @property
    def closed(self):
        return self._plan.closed

    @property
    def plan(self):
        """The stream's `TextPlan` (integers only)."""
        return self._plan

    @property
    def durations(self):
        """Frames of every token of the encoded blocks (host ints)."""
        return list(self._plan.durations)

    @property
    def marks(self):
        """The z-frame at which every encoded token starts, then the frames so far: once finished, what
        `infer_stream(marks=True)` calls `marks`."""
        return list(self._plan.marks)

    @property
    def frames(self):
        """T, once the text is closed and every block is encoded (None before)."""
        return self._plan.total

    @property
    def z_frames(self):
        """z frames flowed so far: z[:, :, :z_frames] is final."""
        return self._plan.z_done

    @property
    def chunks(self):
        return tuple(self._chunks)

    @property
    def failed(self):
        return self._error is not None

    @property
    def finished(self):
        return self.failed or (self._plan.all_released and self._next >= self._decoded)

    def push(self, ids):
        """Appends tokens: ints, a sequence of ints or a 1-D int64 tensor."""
        if torch.is_tensor(ids):
            if ids.dtype != torch.int64 or ids.dim() != 1:
                raise TypeError("push takes ints or a 1-D int64 tensor of token ids")
            ids = ids.tolist()
        elif isinstance(ids, (int, np.integer)) and not isinstance(ids, bool):
            ids = [int(ids)]
        else:
            ids = list(ids)
            if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in ids):
                raise TypeError("push takes ints or a 1-D int64 tensor of token ids")
            ids = [int(v) for v in ids]
        if self._plan.closed:
            raise ValueError("push after close()")
        if len(self._ids) + len(ids) > self.max_tokens:
            raise ValueError("push: %d + %d tokens exceed the stream's capacity of %d (max_tokens)"
                             % (len(self._ids), len(ids), self.max_tokens))
        if any(not -(1 << 63) <= v < 1 << 63 for v in ids):
            raise ValueError("push: a token id outside int64")
        self._ids += ids
        self._plan.push(len(ids))

    def close(self):
        self._plan.close()
        if self._plan.complete and self._plan.frames < 1 and not self.failed:
            self._fail(ValueError("infer_live: the text has no frames (every duration is 0)"))

    # ---- what a pool shares (StreamPool.step); poll() is the stand-alone form of the same steps
    def _check_handle(self):
        if self._net._handle is not self._h:
            raise RuntimeError("the model's handle was re-created (device move) since this stream started")

    def _fail(self, error):
        self._error = error

    def _due_blocks(self):
        return []                     # (no audio to convert: the token blocks go through `_text_tick`)

    def _fill_chunk(self, k, first, count):
        """-> the route length, as a live recording's: the class an utterance of more than 256 frames is decoded in."""
        t = self._plan.t_frames(first, count)      # (what is flowed; with `ahead.dec` the chunk's canonical D)
        k.z, k.z_stride, k.t_frames = self.z.data_ptr(), self.z.stride(1), t
        k.g = self.g.data_ptr() if self.g is not None else None
        k.first, k.o = first, self.o.data_ptr()
        k.count = count + self._plan.overhang(first, count)
        return max(t, 257)

    _fill_seam = LiveStream._fill_seam
    _chunk_decoded = LiveStream._chunk_decoded

    def _next_chunk(self):
        return None if self.failed else self._plan.next_chunk()

    def _drained(self):
        return self.failed or self._plan.all_released

    def poll(self):
        """One tick for this stream alone (the order of `_text_tick`, then every chunk that became decodable: all of
        them in one `mbv_decode_chunks_routed` call, under a seam one call and one `mbv_seam_rows` launch per chunk);
        hands out every chunk not handed out yet: [(first_sample, view), ...].  Raises what failed the stream."""
        if self._error is None:
            _text_tick(self._net, [self])
        if self._error is not None:
            raise self._error
        return _decode_and_hand_out(self)

    def result(self):
        """o[:, :, :spf T] of the finished stream."""
        if self.failed:
            raise self._error
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
    member with nothing decodable yet is skipped and stays, and its next `poll()` hands the pooled chunks out.

    A `TextStream` is a member too: `step()` runs the due token blocks of all text members through shared encoder
    runs, one take launch per run, one read-back, one expand launch and the planned flow runs (`_text_tick`, DESIGN
    §7.27), then decodes at most one chunk of each along with the others'.  A text member that fails (a flagged token
    id, a block that does not fit `max_frames`) is dropped, the others are served; its own `poll()` raises."""

    def __init__(self, net):
        self._net = net
        self.streams = []

    def __len__(self):
        return len(self.streams)

    def add(self, st):
        if not isinstance(st, (DecodeStream, LiveStream, TextStream)):
            raise TypeError("StreamPool.add takes a DecodeStream (net.dec_stream / net.infer_stream), a LiveStream "
                            "(net.convert_live) or a TextStream (net.infer_live)")
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
        if _text_tick(net, [st for st in members if isinstance(st, TextStream)]):
            # a text stream that failed in this tick is dropped; the others are served
            self.streams = [st for st in self.streams if not st._drained()]
            members = [st for st in members if not st._drained()]
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
