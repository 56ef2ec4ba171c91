"""The voices' C entries through ctypes alone, as a binding of `include/mbistft_vits.h` would use them: two voices in
one `mbv_speakers_define` call, read back with `mbv_speaker_embedding`."""
import ctypes as C

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi

import speaker_ref
from gpu_util import make_net, ptr

pytestmark = pytest.mark.gpu

NS, GIN = 12, 256


def test_define_read_back_release():
    net = make_net("uudb_ms_istft_vits_ms")[0]
    h, L, s = net._ensure_handle(), _capi.lib(), net._stream()
    table = net.emb_g.weight.detach().cpu().numpy().astype(np.float64)
    assert L.mbv_speaker_slots() == 256 and L.mbv_speaker_runs(h) == 0
    for sid in (0, NS - 1, NS, NS + 40, NS + 255, NS + 256, -1):
        assert L.mbv_speaker_defined(h, sid) == 0                              # nothing defined yet; real speakers are not voices
    given = torch.randn(GIN, generator=torch.Generator().manual_seed(1)).cuda()
    defs = (_capi.MbvSpeakerDef * 2)()
    defs[0].slot, defs[0].count = 40, 3
    for j, (i, w) in enumerate(((2, 0.5), (11, 0.75), (6, -0.25))):
        defs[0].ids[j], defs[0].weights[j] = i, w
    defs[1].slot, defs[1].vector = 255, given.data_ptr()
    assert L.mbv_speakers_define(h, defs, 2, s) == 0, L.mbv_last_error(h)
    assert L.mbv_speaker_runs(h) == 1                                          # two voices, one launch
    assert L.mbv_speaker_defined(h, NS + 40) == 1 and L.mbv_speaker_defined(h, NS + 255) == 1
    assert L.mbv_speaker_defined(h, NS + 41) == 0 and L.mbv_speaker_defined(h, 2) == 0
    sid = torch.tensor([NS + 255, 5, NS + 40], dtype=torch.int64).cuda()
    out = torch.empty(3, GIN, device="cuda")
    assert L.mbv_speaker_embedding(h, ptr(sid), 3, ptr(out), s) == 0
    assert torch.equal(out[0], given) and torch.equal(out[1], net.emb_g.weight[5])
    ids, w = [2, 11, 6], [0.5, 0.75, -0.25]
    err = np.abs(out[2].cpu().numpy().astype(np.float64) - speaker_ref.blend(table, ids, w))
    assert np.all(err <= speaker_ref.bound(table, ids, w))
    # refusals leave the handle usable and say why
    bad = (_capi.MbvSpeakerDef * 1)()
    bad[0].slot, bad[0].count = 256, 1
    bad[0].weights[0] = 1.0
    assert L.mbv_speakers_define(h, bad, 1, s) != 0
    assert b"slot 256 outside [0, 256)" in L.mbv_last_error(h)
    for slot, count, i0, w0, text in ((7, 0, 0, 1.0, b"0 terms outside [1, 16]"), (7, 17, 0, 1.0, b"17 terms"),
                                      (7, 1, NS, 1.0, b"speaker id 12 outside [0, 12)"),
                                      (7, 1, 0, float("inf"), b"not finite"), (-1, 1, 0, 1.0, b"slot -1 outside")):
        bad[0].slot, bad[0].count, bad[0].ids[0], bad[0].weights[0] = slot, count, i0, w0
        assert L.mbv_speakers_define(h, bad, 1, s) != 0
        assert text in L.mbv_last_error(h), (text, L.mbv_last_error(h))
    twice = (_capi.MbvSpeakerDef * 2)()
    for d in twice:
        d.slot, d.count, d.weights[0] = 9, 1, 1.0
    assert L.mbv_speakers_define(h, twice, 2, s) != 0 and b"named twice" in L.mbv_last_error(h)
    assert L.mbv_speaker_release(h, 256, s) != 0 and b"slot 256 outside [0, 256)" in L.mbv_last_error(h)
    assert L.mbv_speaker_release(h, 7, s) != 0 and b"not defined" in L.mbv_last_error(h)
    assert L.mbv_speaker_runs(h) == 1 and L.mbv_speaker_defined(h, NS + 7) == 0
    # release: undefined at once on the host, in stream order on the device; the other voice stays
    assert L.mbv_speaker_release(h, 40, s) == 0
    assert L.mbv_speaker_defined(h, NS + 40) == 0 and L.mbv_speaker_defined(h, NS + 255) == 1
    assert L.mbv_speaker_release(h, 40, s) != 0
    assert L.mbv_speaker_embedding(h, ptr(sid), 3, ptr(out), s) == 0
    assert torch.equal(out[0], given) and torch.equal(out[2], net.emb_g.weight[0])     # no `bad` here: row 0, hosts check
