"""The packed column axis of a "tail_once" launch, host side (no GPU): `mbv_tail_pack_table` returns the block table the
device builds (one `__host__ __device__` arithmetic for both), checked here against the layout's own rules."""
import ctypes as C

import pytest

from mb_istft_vits_amd import _capi

BN = 384


def table(lens, num, reach, T, halo, pad_right):
    L = _capi.lib()
    arr = (C.c_int64 * len(lens))(*lens)
    n = L.mbv_tail_pack_table(arr, len(lens), num, reach, T, halo, pad_right, BN, None, 0)
    assert n > 0
    out = (C.c_int32 * n)()
    assert L.mbv_tail_pack_table(arr, len(lens), num, reach, T, halo, pad_right, BN, out, n) == n
    assert L.mbv_tail_pack_table(arr, len(lens), num, reach, T, halo, pad_right, BN, out, n - 1) == -1
    return list(out)


def lengths(B, Tz, kind):
    """Lengths in z-frames: 0, 1, a multiple of 32, Tz, donor ties; the donor first or last."""
    base = [Tz, 0, 1, 32, 96, Tz - 1, 7, 0, 33, Tz // 2]
    lens = [base[i % len(base)] + (i // len(base)) % 5 * 3 for i in range(B)]
    lens = [min(Tz, v) for v in lens]
    if kind == "donor_first":
        lens[0] = 0
    elif kind == "donor_last":
        lens = [max(v, 2) for v in lens]
        lens[-1] = 1
    elif kind == "all_equal":
        lens = [Tz] * B
    return lens


@pytest.mark.parametrize("halo,gap", [(2, 32), (50, 64)])
@pytest.mark.parametrize("B", [1, 2, 5, 64])
@pytest.mark.parametrize("kind", ["ties", "donor_first", "donor_last", "all_equal"])
@pytest.mark.parametrize("num,reach,Tz", [(1, 3, 767), (4, 78, 192), (16, 378, 40)])
def test_table_layout(halo, gap, B, kind, num, reach, Tz):
    T = num * Tz
    pad_right = halo - halo // 2
    lens = lengths(B, Tz, kind)
    out = table(lens, num, reach, T, halo, pad_right)
    tiles, donor, used = out[0], out[1], out[2]
    assert donor == lens.index(min(lens))             # lowest index on ties
    sp = out[4:4 + B]
    for b in range(B):
        s = min(T, lens[b] * num + reach)
        want = T if b == donor else min(T, -(-s // 32) * 32)
        assert sp[b] == want, (b, sp[b], want)
        assert sp[b] % 32 == 0 or sp[b] == T
    assert sp[donor] == T                             # the donor is whole
    at = (4 + B + 3) // 4 * 4
    ent = [tuple(out[at + 4 * i: at + 4 * i + 4]) for i in range((len(out) - at) // 4)]
    # the test's own arithmetic: a region of ceil(S' / 32) blocks and a gap of `gap` columns per row, in row order
    assert used == sum(-(-s // 32) + gap // 32 for s in sp)
    assert tiles == -(-used // (BN // 32))
    assert len(ent) >= (tiles + 1) * (BN // 32)       # a window reaching past the last tile finds empty blocks
    seen = [set() for _ in range(B)]
    i = 0
    for b in range(B):                                # every block has one owner; rows in order, starts 32-aligned
        n_out = -(-sp[b] // 32)
        for k in range(n_out):
            row, c0, lim, kind_ = ent[i]
            assert (row, c0, lim, kind_) == (b, 32 * k, sp[b] + pad_right, 1)
            cols = range(c0, min(c0 + 32, sp[b]))
            assert not seen[b] & set(cols)
            seen[b] |= set(cols)
            i += 1
        for k in range(gap // 32):                    # the gap continues the row's columns: its right halo, then zeros
            row, c0, lim, kind_ = ent[i]
            assert (row, c0, lim, kind_) == (b, 32 * (n_out + k), sp[b] + pad_right, 0)
            i += 1
        assert gap >= halo and lim - sp[b] == pad_right and gap - pad_right >= halo - pad_right
    assert i == used
    for b in range(B):                                # every output column of every row exactly once
        assert seen[b] == set(range(sp[b]))
    assert all(e == (0, 0, 0, 0) for e in ent[used:])


def test_bad_arguments():
    L = _capi.lib()
    arr = (C.c_int64 * 2)(3, 4)
    assert L.mbv_tail_pack_table(None, 2, 1, 3, 100, 6, 3, BN, None, 0) == -1
    assert L.mbv_tail_pack_table(arr, 0, 1, 3, 100, 6, 3, BN, None, 0) == -1
    assert L.mbv_tail_pack_table(arr, 2, 1, 3, 100, 6, 7, BN, None, 0) == -1     # pad_right > halo
    assert L.mbv_tail_pack_table(arr, 2, 1, 3, 100, 6, 3, 100, None, 0) == -1    # tile width not a multiple of 32
