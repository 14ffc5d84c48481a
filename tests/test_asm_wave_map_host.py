"""The wave map of the node assembly kernel's two launches (option asm_node_lines), checked on the host.

pph_asm_wave_map runs the library's own map builder (the function the assembly uses) without touching a device.  What the
two launches rely on is restated here and checked over a sweep of boxes and random `near` sets:

  * windows u pairs cover every row of the box and the padding rows up to the next multiple of 64 - no gap;
  * every lane of a straight-line window is `inner` (inside the box, `near` 0): that body has no predicate;
  * a window starts at a multiple of the alignment (an even number of rows; 8 by default) and stays below n; a pair starts at an even row (lanes 2i / 2i + 1 share one 16-byte
    store), pairs ascend and are padded to whole waves of 32 with copies of the last one;
  * the general launch holds only what it must: every pair has a row no window covers;
  * a wave of 64 aligned rows that is all inner (straight-line in the aligned map, asm_node_lines 0) is covered by windows,
    so no row moves from the straight-line to the general form.
"""
import ctypes as C

import numpy as np
import pytest

from perphil_amd import _ffi

DEFAULT_ALIGN = 8       # PPH_N2_WIN_ALIGN: rows (64 bytes of a slot array)


def wave_map(dim, px, py, pz, near, align=1):
    counts = (C.c_int64 * 2)()
    nearp = None if near is None else near.ctypes.data_as(C.c_void_p)
    assert _ffi.lib.pph_asm_wave_map(dim, px, py, pz, align, nearp, None, None, counts) == 0
    win = np.zeros(max(counts[0], 1), dtype=np.uint32)
    pairs = np.zeros(max(counts[1], 1), dtype=np.uint32)
    c2 = (C.c_int64 * 2)()
    assert _ffi.lib.pph_asm_wave_map(dim, px, py, pz, align, nearp, win.ctypes.data_as(C.c_void_p),
                                     pairs.ctypes.data_as(C.c_void_p), c2) == 0
    assert (c2[0], c2[1]) == (counts[0], counts[1])
    return win[:counts[0]].astype(np.int64), pairs[:counts[1]].astype(np.int64)


def inner_rows(dim, px, py, pz, near):
    if dim == 2:
        pz = 1
    n = px * py * pz
    r = np.arange(n)
    gi, gj, gk = r % px, (r // px) % py, r // (px * py)
    inner = (gi > 0) & (gi < px - 1) & (gj > 0) & (gj < py - 1)
    if dim == 3:
        inner &= (gk > 0) & (gk < pz - 1)
    if near is not None:
        inner &= near == 0
    return inner


def check_map(dim, px, py, pz, near, align=1):
    if dim == 2:
        pz = 1
    n = px * py * pz
    n64 = (n + 63) // 64 * 64
    win, pairs = wave_map(dim, px, py, pz, near, align)
    step = DEFAULT_ALIGN if align == 1 else align
    inner = inner_rows(dim, px, py, pz, near)
    tag = f"dim {dim} box {px} x {py} x {pz} align {align}"
    cov = np.zeros(n64, dtype=bool)
    if len(win):
        assert (win % step == 0).all(), tag
        assert (win + 64 <= n).all(), tag
        assert (np.diff(win) > 0).all(), tag
        rows = (win[:, None] + np.arange(64)[None, :]).ravel()
        assert inner[rows].all(), f"{tag}: a window lane is not inner"
        cov[rows] = True
    assert len(pairs) % 32 == 0 and len(pairs) > 0, tag
    assert (pairs % 2 == 0).all() and (pairs + 1 < n64).all(), tag
    assert (np.diff(pairs) >= 0).all(), tag
    d = np.diff(pairs)
    assert (d[: len(pairs) - 32] > 0).all(), f"{tag}: a repeated pair outside the last wave's padding"
    gen = np.zeros(n64, dtype=bool)
    gen[pairs] = True
    gen[pairs + 1] = True
    assert (cov | gen).all(), f"{tag}: rows {np.flatnonzero(~(cov | gen))[:8]} belong to neither launch"
    assert (~cov[pairs] | ~cov[pairs + 1]).all(), f"{tag}: a pair of the general launch that the windows cover"
    # the aligned map's straight-line waves stay straight-line
    full = np.zeros(n64, dtype=bool)
    full[:n] = inner
    aligned = full.reshape(-1, 64).all(axis=1)
    assert cov.reshape(-1, 64)[aligned].all(), tag
    return int(cov.sum()), int(gen[:n].sum())


def random_near(rng, n, mode):
    if mode == 0:
        return None
    near = np.zeros(n, dtype=np.uint8)
    if mode == 1:       # scattered single rows
        near[rng.integers(0, n, size=max(1, n // 500))] = 1
    elif mode == 2:     # a few contiguous stretches (a constrained patch and the rows next to it)
        for _ in range(4):
            a = int(rng.integers(0, n))
            near[a:a + int(rng.integers(1, 200))] = 1
    else:               # dense
        near[rng.random(n) < 0.3] = 1
    return near


def sweep_boxes():
    rng = np.random.default_rng(20240)
    boxes = []
    for p in (3, 4, 33, 34, 64, 65, 66, 67, 68, 69, 70):      # the sizes around one window per line
        boxes.append((p, 5, 4))
        boxes.append((5, p, 3))
        boxes.append((4, 5, p))
    for _ in range(60):
        boxes.append(tuple(int(v) for v in rng.integers(3, 71, size=3)))
    boxes += [(70, 70, 70), (129, 7, 5), (130, 6, 4), (131, 5, 5), (257, 5, 4), (193, 4, 6), (258, 4, 3)]
    return boxes


@pytest.mark.parametrize("dim", [3, 2])
def test_windows_and_pairs_cover_every_row_once_inner_even_adjacent(dim):
    rng = np.random.default_rng(7 + dim)
    for (px, py, pz) in sweep_boxes():
        n = px * py * (pz if dim == 3 else 1)
        for mode in range(4):
            near = random_near(rng, n, mode)
            for align in (1, 2, 16):
                check_map(dim, px, py, pz, near, align)


def test_general_launch_holds_the_boundary_rows_only():
    """A free 129^3 box: 2.02 waves per line.  The aligned map sends about half of the rows through the general form; the
    line map the two outermost nodes of each line end, the boundary lines and planes: under 10 %."""
    p = 129
    n = p ** 3
    win_rows, gen_rows = check_map(3, p, p, p, None)
    inner = inner_rows(3, p, p, p, None)
    assert win_rows >= inner.sum() - 2 * (DEFAULT_ALIGN - 1) * (p - 2) ** 2      # per line: less than one alignment step at either end
    assert gen_rows <= 0.20 * n
    win2, gen2 = check_map(3, p, p, p, None, 2)
    assert win2 >= inner.sum() - (p - 2) ** 2              # even first rows: at most one inner row per line left out
    assert gen2 <= 0.10 * n
    full = np.zeros((n + 63) // 64 * 64, dtype=bool)
    full[:n] = inner
    assert full.reshape(-1, 64).all(axis=1).sum() * 64 <= 0.55 * n


def test_a_line_with_a_near_row_keeps_windows_on_both_sides():
    px, py, pz = 200, 3, 3
    near = np.zeros(px * py * pz, dtype=np.uint8)
    line = (1 * py + 1) * px
    near[line + 100] = 1
    win, pairs = wave_map(3, px, py, pz, near, 2)
    assert list(win) == [line + 2, line + 36, line + 102, line + 134]
    assert line + 100 in set(pairs) and line + 198 in set(pairs) and line in set(pairs)
    check_map(3, px, py, pz, near, 2)
    win, pairs = wave_map(3, px, py, pz, near)
    assert list(win) == [line + 8, line + 32, line + 104, line + 128]


def test_rejects_boxes_beyond_32_bit_row_offsets():
    counts = (C.c_int64 * 2)()
    assert _ffi.lib.pph_asm_wave_map(3, 1024, 1024, 512, 1, None, None, None, counts) != 0
    assert _ffi.lib.pph_asm_wave_map(4, 8, 8, 8, 1, None, None, None, counts) != 0
    assert _ffi.lib.pph_asm_wave_map(3, 8, 8, 8, 6, None, None, None, counts) != 0       # alignment: a power of two up to 64
