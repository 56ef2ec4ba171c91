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
"""
import ctypes as C

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


def decoder_context(config_struct):
    """(L, R) of `mbv_decoder_context` for an `_capi.MbvConfig` (host only)."""
    out = (C.c_int32 * 2)()
    if _capi.lib().mbv_decoder_context(C.byref(config_struct), C.byref(out)):
        raise _capi.MbvError("mbv_decoder_context: unsupported decoder %d" % config_struct.decoder)
    return int(out[0]), int(out[1])


class DecodeStream:
    """Iterator over (first_sample, o[:, :, a:b]) of one decode, one `mbv_decode_range` launch per chunk.

    `o` [B, 1, spf T'] is allocated once, before the first chunk; chunk i is decoded when the iterator reaches it,
    on the caller's current stream at that moment, and its view is ordered on that stream like every other output.
    All state lives in tensors the stream owns (z, g, o), so a paused stream survives other calls on the same model
    (`infer`, `dec`, another stream).  `y_lengths` is set by `infer_stream`."""

    def __init__(self, net, handle, z, g, chunk_frames, max_chunk_frames):
        self._net, self._h = net, handle
        self.z, self.g = z, g
        B, _, Tp = z.shape
        self.spf = net.cfg.samples_per_frame
        self.schedule = chunk_schedule(Tp, chunk_frames, max_chunk_frames)
        self.o = torch.empty(B, 1, self.spf * Tp, device=z.device, dtype=torch.float32)
        self.y_lengths = None
        self._next = 0

    def __len__(self):
        return len(self.schedule)

    def __iter__(self):
        return self

    def __next__(self):
        if self._next >= len(self.schedule):
            raise StopIteration
        first, count = self.schedule[self._next]
        net, h = self._net, self._h
        if net._handle is not h:
            raise RuntimeError("the model's handle was re-created (device move) since this stream started")
        B, _, Tp = self.z.shape
        with torch.cuda.device(self.z.device), torch.no_grad():
            net._ensure_handle()                  # (re-uploads weights edited in place, as every entry does)
            _capi.check(h, _capi.lib().mbv_decode_range(h, net._ptr(self.z), net._ptr(self.g), B, Tp, first, count,
                                                        net._ptr(self.o), self.o.stride(0), net._stream()),
                        "mbv_decode_range")
        self._next += 1
        a, b = self.spf * first, self.spf * (first + count)
        return a, self.o[:, :, a:b]

    def run(self):
        """Decode every remaining chunk; -> o."""
        for _ in self:
            pass
        return self.o
