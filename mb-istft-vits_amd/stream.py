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
        with torch.cuda.device(self.z.device), torch.no_grad():
            net._ensure_handle()                  # (re-uploads weights edited in place, as every entry does)
            _capi.check(h, _capi.lib().mbv_decode_range(h, net._ptr(self.z), net._ptr(self.g), B, Tp, first, count,
                                                        net._ptr(self.o), self.o.stride(0), net._stream()),
                        "mbv_decode_range")
        self._next += 1
        self._decoded = self._next
        return a, self.o[:, :, a:b]

    def run(self):
        """Decode every remaining chunk; -> o."""
        for _ in self:
            pass
        return self.o


class StreamPool:
    """The next chunk of many `DecodeStream`s of one model in one `mbv_decode_chunks` call per `step()`.

    The pool only shares launches; it does not schedule.  `step()` decodes the next not yet decoded chunk of every
    pooled stream that has one (or of those named) and returns `[(st, first_sample, view), ...]`; the chunks count as
    decoded ahead on their streams, so `next(st)` — and a `wire.PcmStream` over `st` — afterwards hands them out
    without a launch.  A stream may be advanced through the pool, alone, or both in turn.  Streams may be added at
    any time, one by one (`add`) or as the requests they come from (`admit`); finished ones drop out."""

    def __init__(self, net):
        self._net = net
        self.streams = []

    def __len__(self):
        return len(self.streams)

    def add(self, st):
        if not isinstance(st, DecodeStream):
            raise TypeError("StreamPool.add takes a DecodeStream (net.dec_stream / net.infer_stream)")
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

    def step(self, streams=None):
        if streams is None:
            members = list(self.streams)
        else:
            members = list(streams)
            for st in members:
                if not any(st is m for m in self.streams):
                    raise ValueError("step(streams=...) names a stream that is not in the pool")
        self.streams = [st for st in self.streams if st._decoded < len(st.schedule)]
        members = [st for st in members if st._decoded < len(st.schedule)]
        if not members:
            return []
        net = self._net
        arr = (_capi.MbvChunk * len(members))()
        out = []
        for k, st in zip(arr, members):
            if net._handle is not st._h:
                raise RuntimeError("the model's handle was re-created (device move) since a pooled stream started")
            first, count = st.schedule[st._decoded]
            k.z, k.z_stride, k.t_frames = st.z.data_ptr(), st.z.stride(1), st.z.shape[2]
            k.g = st.g.data_ptr() if st.g is not None else None
            k.first, k.count, k.o = first, count, st.o.data_ptr()
            out.append((st, st.spf * first, st.o[:, :, st.spf * first:st.spf * (first + count)]))
        dev = net._device()
        with torch.cuda.device(dev), torch.no_grad():
            h = net._ensure_handle()
            _capi.check(h, _capi.lib().mbv_decode_chunks(h, arr, len(members), net._stream()), "mbv_decode_chunks")
        for st in members:
            st._decoded += 1
        self.streams = [st for st in self.streams if st._decoded < len(st.schedule)]
        return out
