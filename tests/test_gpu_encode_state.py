"""State the C entries keep between calls ("What an entry keeps"): an encode run and a stage reference end
when anything lays out the scratch they point into, and an entry that is given an ended run refuses before it launches.

The Python layer never makes these sequences, so the tests drive the C entries.  No buffer regrows between making a
run and using it here (every later claim of that buffer is smaller), so an implementation that did launch on an
ended run would read overwritten, still allocated memory and fail these assertions without faulting the card."""
import ctypes as C

import pytest
import torch

from mb_istft_vits_amd import _capi

from gpu_util import make_net

pytestmark = pytest.mark.gpu

SENT = -77
T_ROWS = (8, 6)                                               # the pooled run: B = 2 rows padded to T = 8


@pytest.fixture(scope="module")
def net():
    return make_net("ljs_mini_mb_istft_vits")[0]


def _ids(B, T, seed):
    return torch.randint(1, 59, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


def _encode_rows(net, slot, seed=1):
    """mbv_encode_rows(slot) of T_ROWS at length_scale 1 -> the rows' frame counts"""
    h, L = net._ensure_handle(), _capi.lib()
    B, T = len(T_ROWS), max(T_ROWS)
    ids, lens = _ids(B, T, seed), torch.tensor(T_ROWS).cuda()
    for b, t in enumerate(T_ROWS):
        ids[b, t:] = 0
    rows = (_capi.MbvEncRow * B)()
    for row, t in zip(rows, T_ROWS):
        row.length_scale, row.noise_scale_w, row.t_text = 1.0, 0.0, t
    y = torch.full((B,), SENT, dtype=torch.int64).cuda()
    rc = L.mbv_encode_rows(h, slot, ids.data_ptr(), lens.data_ptr(), None, B, T, rows, y.data_ptr(), None)
    assert rc == 0, L.mbv_last_error(h)
    frames = y.tolist()
    assert all(f >= t for f, t in zip(frames, T_ROWS)), frames
    return frames


def _encode(net, B=1, T=4, seed=2):
    """the plain mbv_encode of B full rows of T tokens"""
    h, L = net._ensure_handle(), _capi.lib()
    ids, lens = _ids(B, T, seed), torch.full((B,), T).cuda()
    y = torch.full((B,), SENT, dtype=torch.int64).cuda()
    rc = L.mbv_encode(h, ids.data_ptr(), lens.data_ptr(), None, B, T, 1.0, None, 1.0, y.data_ptr(), None)
    assert rc == 0, L.mbv_last_error(h)
    torch.cuda.synchronize()


class RowsCalls:
    """The four `_rows` entries on one slot of a T_ROWS run, every output pre-filled with SENT."""

    def __init__(self, net, slot, frames):
        self.h, self.L, self.slot, self.frames = net._ensure_handle(), _capi.lib(), slot, list(frames)
        B, I = len(T_ROWS), net.cfg.inter_channels
        dev = "cuda"
        self.z = [torch.full((1, I, f), float(SENT), device=dev) for f in frames]
        self.marks = [torch.full((t + 1,), SENT, dtype=torch.int64, device=dev) for t in T_ROWS]
        self.y = torch.full((B,), SENT, dtype=torch.int64, device=dev)
        self.gain_out = [torch.full((f + 1,), float(SENT), device=dev) for f in frames]
        self.tables = [torch.full((t,), 1.5, device=dev) for t in T_ROWS]      # a scale or a gain per token
        self.syn = (_capi.MbvRow * B)()
        self.mark = (_capi.MbvMarkRow * B)()
        self.shape = (_capi.MbvShapeRow * B)()
        self.gain = (_capi.MbvGainRow * B)()
        for b in range(B):
            self.syn[b].noise_stride, self.syn[b].noise_scale = frames[b], 0.0
            self.syn[b].keep, self.syn[b].z = frames[b], self.z[b].data_ptr()
            self.mark[b].marks, self.mark[b].count = self.marks[b].data_ptr(), T_ROWS[b] + 1
            self.shape[b].scale = self.tables[b].data_ptr()
            self.gain[b].gain, self.gain[b].out = self.tables[b].data_ptr(), self.gain_out[b].data_ptr()
            self.gain[b].frames = frames[b]

    def calls(self):
        h, L, k, B = self.h, self.L, self.slot, len(T_ROWS)
        return {"mbv_token_marks_rows": lambda: L.mbv_token_marks_rows(h, k, self.mark, B, None),
                "mbv_frame_gain_rows": lambda: L.mbv_frame_gain_rows(h, k, self.gain, B, None),
                "mbv_shape_durations_rows": lambda: L.mbv_shape_durations_rows(h, k, self.shape, B, self.y.data_ptr(), None),
                "mbv_synthesize_rows": lambda: L.mbv_synthesize_rows(h, k, max(self.frames), self.syn, B, None)}

    def outputs(self):
        return self.z + self.marks + [self.y] + self.gain_out

    def assert_all_refused(self, needle):
        shape_runs, gain_runs = self.L.mbv_shape_runs(self.h), self.L.mbv_gain_runs(self.h)
        for name, call in self.calls().items():
            assert call() != 0, name
            err = self.L.mbv_last_error(self.h)
            assert name.encode() in err and needle in err, (name, err)
        torch.cuda.synchronize()
        for t in self.outputs():
            assert (t == SENT).all(), "a refused entry wrote an output"
        assert self.L.mbv_shape_runs(self.h) == shape_runs and self.L.mbv_gain_runs(self.h) == gain_runs


def _assert_slot0_accepts_then(net, end_the_run):
    """The four `_rows` entries take a slot-0 run; after `end_the_run()` has laid out its scratch they refuse it."""
    # not vacuous: these very arguments are accepted (the scale tables first: the other three take the frames they leave)
    shaped = RowsCalls(net, 0, _encode_rows(net, 0))
    assert shaped.calls()["mbv_shape_durations_rows"]() == 0, shaped.L.mbv_last_error(shaped.h)
    frames = shaped.y.tolist()
    assert all(f >= t for f, t in zip(frames, T_ROWS)), frames
    ok = RowsCalls(net, 0, frames)
    for name, call in ok.calls().items():
        if name != "mbv_shape_durations_rows":
            assert call() == 0, (name, ok.L.mbv_last_error(ok.h))
    torch.cuda.synchronize()
    assert all(not (t == SENT).any() for t in ok.z + ok.marks + ok.gain_out)
    frames = _encode_rows(net, 0)
    end_the_run()
    RowsCalls(net, 0, frames).assert_all_refused(b"slot 0")


def test_a_plain_encode_ends_the_run_of_slot_0(net):
    _assert_slot0_accepts_then(net, lambda: _encode(net))


def test_align_ends_the_run_of_slot_0_and_the_plain_state(net):
    def align():
        x, y = _ids(1, 4, 3), torch.rand(1, net.cfg.spec_channels, 12, generator=torch.Generator().manual_seed(4)).cuda() + 0.1
        w = net.align(x, torch.tensor([4]).cuda(), y, torch.tensor([12]).cuda(), noise_scale=0, outputs=("w",))[1]
        assert int(w.sum()) == 12

    _assert_slot0_accepts_then(net, align)
    h, L = net._ensure_handle(), _capi.lib()
    marks = torch.full((2, 9), SENT, dtype=torch.int64).cuda()
    assert L.mbv_token_marks(h, marks.data_ptr(), 9, None) != 0
    assert b"mbv_token_marks without a preceding mbv_encode" in L.mbv_last_error(h)
    torch.cuda.synchronize()
    assert (marks == SENT).all()


def test_a_slot_with_its_own_buffer_outlives_a_plain_encode(net):
    got = []
    for between in (False, True):
        frames = _encode_rows(net, 1, seed=5)
        if between:
            _encode(net)
        run = RowsCalls(net, 1, frames)
        assert run.calls()["mbv_synthesize_rows"]() == 0, run.L.mbv_last_error(run.h)
        torch.cuda.synchronize()
        got.append((frames, run.z))
    assert got[0][0] == got[1][0]
    for a, b in zip(got[0][1], got[1][1]):
        assert torch.isfinite(a).all() and not (a == SENT).any() and torch.equal(a, b)


def test_slot_0_and_the_plain_state_are_one(net):
    h, L = net._ensure_handle(), _capi.lib()
    _encode(net, B=2, T=8)
    run = RowsCalls(net, 0, [8, 8])
    run.assert_all_refused(b"slot 0 holds no mbv_encode_rows run")
    _encode_rows(net, 0)
    y = torch.full((2,), SENT, dtype=torch.int64).cuda()
    scale = torch.full((2, 8), 1.5).cuda()
    runs = L.mbv_shape_runs(h)
    assert L.mbv_shape_durations(h, scale.data_ptr(), None, None, 2, 8, None, y.data_ptr(), None) != 0
    assert b"the last encode was mbv_encode_rows" in L.mbv_last_error(h)
    torch.cuda.synchronize()
    assert (y == SENT).all() and L.mbv_shape_runs(h) == runs


def test_a_stage_ends_with_its_scratch(net):
    x, xl = _ids(2, 8, 6), torch.tensor([8, 5]).cuda()
    net.infer(x, xl, noise_scale=0, outputs=("o",))
    x_enc, x_post = net.read_stage("x_enc").clone(), net.read_stage("x_post").clone()
    assert x_enc.abs().sum() > 0 and x_post.abs().sum() > 0
    # one pooled wire call that writes a single sample: it lays out the decoder's scratch, not the encoder's
    wave, valid = torch.full((64,), 0.25).cuda(), torch.tensor([64]).cuda()
    pcm, running = torch.full((8,), SENT, dtype=torch.int16).cuda(), torch.zeros(1).cuda()
    k = _capi.MbvPcmChunk()
    k.wave, k.in_total, k.valid_samples = wave.data_ptr(), 64, valid.data_ptr()
    k.in_avail, k.out_first, k.out_count = 64, 0, 1
    k.pcm, k.pcm_capacity, k.running_peak = pcm.data_ptr(), pcm.numel(), running.data_ptr()
    net.resample_pcm16_chunks([k], 22050, 24000)
    torch.cuda.synchronize()
    assert pcm[0] != SENT and (pcm[1:] == SENT).all()
    with pytest.raises(_capi.MbvError, match="stage 'x_post' not available"):
        net.read_stage("x_post")
    assert torch.equal(net.read_stage("x_enc"), x_enc)
