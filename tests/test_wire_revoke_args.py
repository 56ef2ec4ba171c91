"""CPU checks of `wire._revoke_args`, the `fade_ms` / `at` parser that `PcmStream.revoke` and `Turn.revoke` share, on
plain integers: no tensor, no GPU.  The error texts are those the two methods have always raised."""
import re

import numpy as np
import pytest

from mb_istft_vits_amd import wire

RATE = 24000
E, TOTAL = 1000, 5000                      # samples handed out so far, the stream's length
MARKS = [0, 400, 999, 1000, 1800, 4200, TOTAL]
NO_MARKS = ("revoke(at='token'): the stream has no token marks (infer_stream(marks=True); a converted recording has no "
            "tokens)")


def args(fade_ms, at, marks=None, tokens=True, emitted=E, finished=False):
    return wire._revoke_args(fade_ms, at, RATE, emitted, TOTAL, marks, tokens, finished)


def refused(text, *a, **kw):
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        args(*a, **kw)


def test_accepted_forms():
    assert args(5.0, "now") == (E, 120)                                    # N = round(fade_ms * rate / 1000)
    assert args(5.0, "now", tokens=False) == (E, 120)
    assert args(0, "now") == (E, 0)                                        # a hard cut
    assert args(0.02, "now") == (E, 0) and args(0.03, "now") == (E, 1)     # 0.48 and 0.72 samples, rounded
    assert args(5.0, 1234) == (1234, 120) and args(5.0, 1234, tokens=False) == (1234, 120)
    F, N = args(5.0, np.int64(1234))
    assert (F, N) == (1234, 120) and type(F) is int and type(N) is int
    assert args(2.5, np.int32(7), tokens=False) == (7, 60)
    # (an index below E is parsed: `revoke_plan` refuses it, with both numbers in its message)
    assert args(5.0, E - 1) == (E - 1, 120)
    with pytest.raises(ValueError, match="%d samples have been handed out already" % E):
        wire.revoke_plan([TOTAL], TOTAL, E, *args(5.0, E - 1))


def test_token_picks_the_first_mark_at_or_after_what_was_handed_out():
    assert args(5.0, "token", MARKS) == (1000, 120)                        # a mark at E itself counts
    assert args(5.0, "token", MARKS, emitted=1001) == (1800, 120)
    assert args(5.0, "token", MARKS, emitted=0) == (0, 120)
    assert args(5.0, "token", MARKS, emitted=4201) == (TOTAL, 120)
    assert args(5.0, "token", [0, 400], emitted=401) == (TOTAL, 120)       # no mark is left: the end of the stream
    assert args(5.0, "token", [], emitted=0) == (TOTAL, 120)


def test_refusals_keep_their_texts():
    for bad in (True, False, 1234.0, 1.5, "later", None, (1, 2)):
        refused("revoke: at must be 'now', 'token' or a wire sample index, got %r" % (bad,), 5.0, bad, MARKS)
        refused("revoke: at must be 'now' or a wire sample index, got %r" % (bad,), 5.0, bad, tokens=False)
    refused(NO_MARKS, 5.0, "token")                                        # a stream without marks
    refused(NO_MARKS, 5.0, "token", None)
    refused("revoke: at must be 'now' or a wire sample index, got 'token'", 5.0, "token", tokens=False)   # a turn
    refused("revoke: at must be 'now' or a wire sample index, got 'token'", 5.0, "token", MARKS, tokens=False)
    for bad in (-1.0, -1e-9, float("nan"), -float("inf")):
        for at in ("now", "token", 1234, "later"):                         # fade_ms is checked first
            refused("revoke: fade_ms must be >= 0", bad, at, MARKS)
            refused("revoke: fade_ms must be >= 0", bad, at, tokens=False)


def test_a_finished_stream_only_has_its_fade_checked():
    assert args(5.0, "later", finished=True) is None and args(5.0, "token", finished=True) is None
    assert args(float("inf"), "now", finished=True) is None
    refused("revoke: fade_ms must be >= 0", -1.0, "now", finished=True)
    refused("revoke: fade_ms must be >= 0", float("nan"), "later", finished=True)
