"""Live voice conversion with a bounded look-ahead, what a cut window computes (no GPU): with the CPU oracle, a
spectrogram window that ends at E, run as one row of a padded run whose length ends there, gives on the frames it keeps
what the whole run gives on the spectrogram cut at E.  The left edge is `mbv_convert_window`'s, so the
left context is that of `test_live_context.py`; the bar is the one used there, the expected difference 0.0."""
import ctypes as C

import pytest
import torch

from mb_istft_vits_amd import _capi

from test_live_context import T, _setup, _z_hat

# (first, count, ahead, final): a block at the start, in the middle, across a 32-frame unit, with no look-ahead at all,
# with the full reach (today's window), clipped by the end of a closed recording, of an open recording
CASES = [(0, 4, 8, T), (128, 8, 8, T), (157, 4, 3, T), (200, 1, 0, T), (64, 32, 96, T), (292, 8, 16, T), (96, 8, 4, 108)]


@pytest.mark.parametrize("name", ["uudb_ms_istft_vits_ms", "ljs_ms_istft_vits"])
def test_a_window_cut_behind_the_block_is_the_recording_cut_there(name):
    net, W, y, noise, g_src, g_tgt, _ = _setup(name)
    cfg_s = net._config_struct()
    out = (C.c_int32 * 2)()
    worst = 0.0
    for first, count, ahead, final in CASES:
        assert _capi.lib().mbv_convert_window_ahead(C.byref(cfg_s), first, count, ahead, final, C.byref(out)) == 0
        wa, E = int(out[0]), int(out[1])
        assert E == min(first + count + ahead, final)
        # the reference: the whole run on the spectrogram cut at E (a recording that ends there), padded to T columns
        # like the window's run below, so that the CPU conv library picks one algorithm for both
        yc, nc = torch.zeros_like(y), torch.zeros_like(noise)
        yc[:, :, :E], nc[:, :, :E] = y[:, :, :E], noise[:, :, :E]
        want = _z_hat(net.cfg, W, yc, nc, g_src, g_tgt, length=E)
        yw, nw = torch.zeros_like(y), torch.zeros_like(noise)
        yw[:, :, :E - wa], nw[:, :, :E - wa] = y[:, :, wa:E], noise[:, :, wa:E]
        got = _z_hat(net.cfg, W, yw, nw, g_src, g_tgt, length=E - wa)
        d = float((got[:, :, first - wa:first - wa + count] - want[:, :, first:first + count]).abs().max())
        print("%s: z_hat[%d, %d) from window [%d, %d): max abs difference to the run cut at %d: %.3g"
              % (name, first, first + count, wa, E, E, d))
        worst = max(worst, d)
    assert worst <= 1e-6
