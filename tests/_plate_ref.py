"""The background plate's rule (include/mdqe_hip.h, above mdqe_plate_update_u8) restated in numpy from the header's text: the oracle of
the plate tests.  Integers only, so every comparison with the device is exact.

A plane of state is (P int64 [h, w, C], n int64 [h, w]): C = 3 for RGB, 1 for luma, 2 for chroma.  `to_state` / `from_state` give the
device's int32 cells: (P_0, P_1, P_2, n), (P, n), (P_U, P_V, n, 0)."""
import numpy as np

TH, TW = 16, 64                                                       # the picture kernel's tile: what "another tile" means below
INTS = {3: 4, 1: 2, 2: 4}


def fresh(h, w, C):
    return np.zeros((h, w, C), dtype=np.int64), np.zeros((h, w), dtype=np.int64)


def from_picture(values):
    """The state an empty-scene shot starts: P = 256 * value, n = 1 everywhere.  values: [h, w, C]."""
    v = np.asarray(values).astype(np.int64)
    return 256 * v, np.ones(v.shape[:2], dtype=np.int64)


def to_state(P, n):
    h, w, C = P.shape
    st = np.zeros((h, w, INTS[C]), dtype=np.int32)
    st[..., :C] = P
    st[..., C] = n
    return st


def from_state(st, C):
    st = np.asarray(st).astype(np.int64)
    assert st.shape[2] == INTS[C] and (C != 2 or not st[..., 3].any())
    return st[..., :C].copy(), st[..., C].copy()


def observed_chroma(block):
    """block [F, H, W] -> bool [F, ceil(H/2), ceil(W/2)]: a chroma pair is observed iff every in-picture pixel of its 2 x 2 block is."""
    F, H, W = block.shape
    pad = np.zeros((F, 2 * ((H + 1) // 2), 2 * ((W + 1) // 2)), dtype=bool)
    pad[:, :H, :W] = block != 0                                       # (pixels beyond the picture do not count)
    return ~pad.reshape(F, pad.shape[1] // 2, 2, pad.shape[2] // 2, 2).any(axis=(2, 4))


def update(P, n, s, obs, N, stats=None):
    """The frames of one call in order.  s: int [F, h, w, C] observed values; obs: bool [F, h, w].  -> (P, n), new arrays.
    stats (a dict): counts what the inputs exercised -- 'floor': observations with a negative numerator and a non-zero remainder;
    'saturated': observations met with n == N already."""
    P, n = P.copy(), n.copy()
    for f in range(s.shape[0]):
        o = np.asarray(obs[f], dtype=bool)
        n1 = np.minimum(n + 1, N)
        num = 256 * s[f].astype(np.int64) - P + (n1 >> 1)[..., None]
        P1 = P + np.floor_divide(num, n1[..., None])                  # floordiv: towards minus infinity
        if stats is not None:
            stats["floor"] = stats.get("floor", 0) + int(((num < 0) & (num % n1[..., None] != 0) & o[..., None]).sum())
            stats["saturated"] = stats.get("saturated", 0) + int(((n == N) & o).sum())
        P = np.where(o[..., None], P1, P)
        n = np.where(o, n1, n)
    return P, n


def _offsets(reach):
    """The offsets of the disc in the order a never-seen pixel prefers them: (d2, dy, dx) ascending = (d2, Y', X') for a fixed pixel."""
    offs = [(dy * dy + dx * dx, dy, dx) for dy in range(-reach, reach + 1) for dx in range(-reach, reach + 1)
            if dy * dy + dx * dx <= reach * reach and (dy, dx) != (0, 0)]
    return sorted(offs)


def sources(n, reach):
    """Where every cell's value comes from, vectorised: int64 [h, w, 2] = (Y', X'); itself where seen, (-1, -1) where `fill` shows."""
    h, w = n.shape
    seen = n > 0
    src = np.full((h, w, 2), -1, dtype=np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    src[seen] = np.stack([yy[seen], xx[seen]], -1)
    todo = ~seen
    for _, dy, dx in _offsets(reach):
        if not todo.any():
            break
        ys, xs = yy + dy, xx + dx
        ok = todo & (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)      # nothing is read beyond the plane
        ok[ok] = seen[ys[ok], xs[ok]]
        src[ok] = np.stack([ys[ok], xs[ok]], -1)
        todo &= ~ok
    return src


def sources_pixelwise(n, reach, ties=None):
    """`sources` pixel by pixel, by brute force over ALL seen cells: the independent form.  ties (a dict): counts the never-seen cells
    whose smallest d2 is shared by candidates of different Y' ('Y') and whose smallest (d2, Y') by several X' ('X')."""
    h, w = n.shape
    sy, sx = np.nonzero(n > 0)
    src = np.full((h, w, 2), -1, dtype=np.int64)
    for Y in range(h):
        for X in range(w):
            if n[Y, X] > 0:
                src[Y, X] = (Y, X)
                continue
            d2 = (sy - Y) ** 2 + (sx - X) ** 2
            ok = d2 <= reach * reach
            if not ok.any():
                continue
            cand = sorted(zip(d2[ok].tolist(), sy[ok].tolist(), sx[ok].tolist()))
            src[Y, X] = cand[0][1:]
            if ties is not None:
                near = [c for c in cand if c[0] == cand[0][0]]
                ties["Y"] = ties.get("Y", 0) + (len({c[1] for c in near}) > 1)
                ties["X"] = ties.get("X", 0) + (sum(1 for c in near if c[1] == near[0][1]) > 1)
    return src


def picture(P, n, reach, fill, src=None):
    """int64 [h, w, C]: (P + 128) >> 8 of the cell `sources` names, `fill` (C ints) where it names none."""
    src = sources(n, reach) if src is None else src
    val = (P + 128) >> 8
    out = np.empty_like(val)
    out[...] = np.asarray(fill, dtype=np.int64)
    has = src[..., 0] >= 0
    out[has] = val[src[has][:, 0], src[has][:, 1]]
    return out


# ---- inputs that can go wrong -----------------------------------------------------------------------------------------------------------
def update_case(seed, F, h, w, C, top, N):
    """(s int64 [F, h, w, C] values 0..top, block uint8 [F, h, w]) holding a pixel that is never free, one that is free in every frame
    (it saturates for N < F), one blocked in some frames and free between them, and blobs that move; asserted here, on the CPU."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, top + 1, size=(F, h, w, C)).astype(np.int64)
    s[:, : h // 2] = np.where(rng.random((F, h // 2, w, 1)) < 0.5, s[:, : h // 2], s[:1, : h // 2])     # (a half that mostly repeats)
    block = np.zeros((F, h, w), dtype=np.uint8)
    for f in range(F):
        for _ in range(3):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            block[f, y0:y0 + int(rng.integers(1, 8)), x0:x0 + int(rng.integers(1, 30))] = rng.integers(1, 256)
    block[:, h - 3:, w - 5:] = 7                                       # never free (the picture's corner: ragged tiles)
    block[:, 0, :3] = 0                                                # always free
    block[:, 1, 1] = [1, 0, 200, 0, 1][:F] if F == 5 else (np.arange(F) % 2 == 0)      # blocked, free, blocked, free, ...
    check_update_case(s, block, N)
    return s, block


def check_update_case(s, block, N, need_floor=None):
    F, h, w = block.shape
    obs = block == 0
    stats = {}
    P, n = update(*fresh(h, w, s.shape[3]), s, obs, N, stats)
    assert (~obs.any(0)).any(), "no pixel is never seen"
    assert not (n[~obs.any(0)]).any() and not P[~obs.any(0)].any()
    if N < F:
        assert stats["saturated"] > 0 and int(n.max()) == N, "no count saturates"
    if N > 1 if need_floor is None else need_floor:                    # (N == 1 divides by one: no remainder)
        assert stats["floor"] > 0, "no negative numerator with a remainder: floor and truncation would agree"
    between = np.zeros((h, w), dtype=bool)
    for a in range(F):
        for b in range(a + 2, F):
            between |= obs[a] & obs[b] & ~obs[a + 1:b].all(0)
    assert between.any(), "no pixel is blocked between two frames that see it"
    assert int(P.min()) >= 0 and int(P.max()) <= 256 * int(s.max())
    return stats


def picture_cases(seed, h, w, C, top):
    """name -> (P, n): states whose pictures can go wrong, asserted here on the CPU (at reach 5; 1 on a plane no higher than a tile): a never-seen cell filled from ANOTHER
    tile (where the plane has more than one), one beyond reach, a d2 tie resolved by Y' and one by X', a plane seen everywhere."""
    rng = np.random.default_rng(seed)

    def state(n):
        P = rng.integers(0, 256 * top + 1, size=(h, w, C)).astype(np.int64)
        P[n == 0] = 0
        return P, n.astype(np.int64)
    cases = {}
    n = rng.integers(1, 70, size=(h, w))
    cases["seen everywhere"] = state(n.copy())
    holes = n.copy()
    y1, x0, x1 = min(h - 2, 30), max(w - 20, 2), w - 3
    holes[4:y1, x0:x1] = 0                                             # a large hole: across tile borders where the plane has them
    if w > TW + 4:
        holes[2:h - 2, TW - 6:TW + 7] = 0                              # ... and one over the column border for certain
    holes[2:h - 3, 10] = 0                                             # a strip one cell wide: (Y, 9) and (Y, 11) tie, the same Y'
    holes[h - 2, 14:min(w - 2, 40)] = 0                                # a strip one cell high: (Y - 1, X) and (Y + 1, X) tie
    holes[:3, :3] = 0                                                  # the plane's corner: nothing is read beyond it
    holes[h - 1, w - 1] = 0
    cases["holes"] = state(holes)
    cases["random"] = state(np.where(rng.random((h, w)) < 0.5, n, 0))
    cases["sparse"] = state(np.where(rng.random((h, w)) < 0.01, n, 0))
    cases["nothing seen"] = state(np.zeros((h, w), dtype=np.int64))
    # what the cases hold
    assert bool((cases["seen everywhere"][1] > 0).all())
    ties = {}
    hn = cases["holes"][1]
    src = sources_pixelwise(hn, 5 if h > TH else 1, ties)             # (a plane no higher than a tile has lower holes: reach 1)
    assert ties.get("Y", 0) > 0 and ties.get("X", 0) > 0, ties
    unseen = hn == 0
    assert (src[unseen][:, 0] < 0).any(), "no cell beyond reach"
    assert (src[unseen][:, 0] >= 0).any()
    if h > TH or w > TW:
        yy, xx = np.nonzero(unseen & (src[..., 0] >= 0))
        sy, sx = src[yy, xx, 0], src[yy, xx, 1]
        assert ((yy // TH != sy // TH) | (xx // TW != sx // TW)).any(), "no cell is filled from another tile"
    return cases


def moving_square(F, h, w, side=6):
    """block [F, h, w]: a square that moves along the diagonal, further per frame than it overlaps itself -- every pixel it covers in
    one frame is free in another."""
    block = np.zeros((F, h, w), dtype=np.uint8)
    for f in range(F):
        y, x = 1 + 2 * f, 2 + 5 * f
        block[f, y:y + side, x:x + side] = 3
    return block
