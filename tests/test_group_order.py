"""Block order of the grouped launches (nk_hartley_sandwich_group): the host copy of the kernels' decode is a bijection of the
grid onto (member, workgroup) pairs that keeps every workgroup on the XCD of its single launch (no compute calls: CPU box)."""
import ctypes

import pytest

from nifty_amd import _lib as L


@pytest.mark.parametrize("per", [1, 7, 8, 9, 25, 1089])
@pytest.mark.parametrize("count", [1, 2, 3, 4])
def test_group_order_is_a_bijection(per, count):
    lib = L.load()
    grid = lib.nk_group_grid_size(per, count)
    assert grid == (per + 7) // 8 * 8 * count
    member, local = ctypes.c_int64(), ctypes.c_int64()
    seen, surplus = set(), 0
    for bid in range(grid):
        assert lib.nk_group_order(bid, count, ctypes.byref(member), ctypes.byref(local)) == L.NK_OK
        m, b = member.value, local.value
        assert 0 <= m < count and b >= 0
        assert b % 8 == bid % 8  # the XCD of the member's single launch
        if b >= per:
            surplus += 1  # leaves at once
            continue
        assert (m, b) not in seen
        seen.add((m, b))
    assert seen == {(m, b) for m in range(count) for b in range(per)}
    assert surplus == grid - per * count


def test_group_members_are_neighbours_in_dispatch_order():
    """The workgroups of all members for one row sit inside one window of 8 * count consecutive workgroups."""
    lib = L.load()
    member, local = ctypes.c_int64(), ctypes.c_int64()
    count, where = 4, {}
    for bid in range(lib.nk_group_grid_size(25, count)):
        lib.nk_group_order(bid, count, ctypes.byref(member), ctypes.byref(local))
        where.setdefault(local.value, []).append(bid)
    for b, bids in where.items():
        assert len(bids) == count and max(bids) - min(bids) == 8 * (count - 1)
        assert len({x // (8 * count) for x in bids}) == 1


def test_group_order_rejects_bad_arguments():
    lib = L.load()
    member, local = ctypes.c_int64(), ctypes.c_int64()
    assert lib.nk_group_order(0, 0, ctypes.byref(member), ctypes.byref(local)) == L.NK_ERR_INVALID
    assert lib.nk_group_order(0, L.MAX_GROUP + 1, ctypes.byref(member), ctypes.byref(local)) == L.NK_ERR_INVALID
    assert lib.nk_group_order(-1, 2, ctypes.byref(member), ctypes.byref(local)) == L.NK_ERR_INVALID
