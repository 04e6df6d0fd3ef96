"""The rule of mdqe_render_blur_within_u8 and mdqe_render_blur_within_yuv420sp (include/mdqe_hip.h) restated in numpy int64: the oracle
of the edge-stopping blur's tests.  Written from the header's text; it shares nothing with the package's torch host path.  Everything
that is not the blurred value is the plain blur's rule, so the source values, the edges and the action tables are those of
tests/_blur_ref.py (and through it tests/_overlay_ref.py / tests/_overlay_yuv_ref.py).  The largest quantity, N, stays below
2^24 * 1023 < 2^34: int64 holds every sum, and `within_loops` uses Python ints throughout.  `within` is vectorised by shifted sums over
an edge-padded copy; `within_loops` is the same rule as plain loops per pixel, the way it is written down, which `within` is checked
against on a small case.  Integers only, so every comparison against it is exact."""
import numpy as np

import _blur_ref as BREF
import _overlay_ref as OREF
import _overlay_yuv_ref as YREF
from _blur_ref import action_tables  # noqa: F401  (the tables of the tests are the plain blur's)


def _sums(t, w, R):
    """t int64 [F, h, w(, C)] -> sum_d w[|d|] * t(Y', X') over rows then columns, clamped coordinates, no rounding."""
    def one(u, axis):
        n = u.shape[axis]
        pad = [(0, 0)] * u.ndim
        pad[axis] = (R, R)
        e = np.pad(u, pad, mode="edge")
        acc = np.zeros_like(u)
        for d in range(-R, R + 1):
            acc += w[abs(d)] * np.take(e, np.arange(R + d, R + d + n), axis=axis)
        return acc
    return one(one(t, 2), 1)


def within(v, member, taps):
    """v int64 [F, h, w(, C)], member bool [F, h, w] -> (N + D // 2) // D where member, 0 elsewhere (the value is not defined there)."""
    w, R = BREF._taps(taps)
    v = np.asarray(v).astype(np.int64)
    m = np.asarray(member).astype(np.int64)
    assert m.shape == v.shape[:3]
    mv = m.reshape(m.shape + (1,) * (v.ndim - 3))
    N, D = _sums(mv * v, w, R), _sums(mv, w, R)
    assert D.max(initial=0) <= 2 ** 24 and (D[mv == 1] >= w[0] ** 2).all()
    return np.where(mv == 1, (N + D // 2) // np.maximum(D, 1), 0)


def within_loops(v, member, taps):
    """`within` as loops over the pixels and the taps in Python ints, with the clamped coordinates of the header."""
    w, R = BREF._taps(taps)
    v = np.asarray(v).astype(np.int64)
    m = np.asarray(member).astype(np.int64)
    flat = v.reshape(v.shape[:3] + (-1,))
    F, H, W, C = flat.shape
    out = np.zeros_like(flat)
    for f in range(F):
        hn = [[[0] * C for _ in range(W)] for _ in range(H)]
        hw = [[0] * W for _ in range(H)]
        for Y in range(H):
            for X in range(W):
                for d in range(-R, R + 1):
                    x = min(max(X + d, 0), W - 1)
                    mm = int(m[f, Y, x])
                    hw[Y][X] += w[abs(d)] * mm
                    for c in range(C):
                        hn[Y][X][c] += w[abs(d)] * mm * int(flat[f, Y, x, c])
                assert hw[Y][X] <= 4096
        for Y in range(H):
            for X in range(W):
                if not m[f, Y, X]:
                    continue
                D, N = 0, [0] * C
                for d in range(-R, R + 1):
                    y = min(max(Y + d, 0), H - 1)
                    D += w[abs(d)] * hw[y][X]
                    for c in range(C):
                        N[c] += w[abs(d)] * hn[y][X][c]
                assert w[0] ** 2 <= D <= 2 ** 24
                for c in range(C):
                    out[f, Y, X, c] = (N[c] + D // 2) // D
    return out.reshape(v.shape)


def paint(labels, frames, palette, action, a256=128, contour=1, taps=(4096,), within_fn=within):
    """RGB -> uint8 [F, Ho, Wo, 3], the arguments of _blur_ref.paint."""
    lab, a = BREF._checked(labels, action, a256, contour)
    F, Ho, Wo = lab.shape
    s = OREF.source_values(frames, F, Ho, Wo)
    col = np.asarray(palette).astype(np.int64)[lab]
    tinted = np.where(OREF.edges(lab, contour)[..., None], col, (s * (256 - a256) + col * a256 + 128) >> 8)
    out = np.where((a == 0)[..., None], s, np.where((a == 3)[..., None], within_fn(s, a == 3, taps), tinted))
    return out.astype(np.uint8)


def paint_yuv(ys, cs, labels, pal_yuv, action, fmt, a256=128, contour=1, taps=(4096,), taps_c=(4096,), within_fn=within):
    """Stored samples in, stored samples out, the arguments of _blur_ref.paint_yuv -> (ys', cs')."""
    p010 = fmt == "p010"
    lab, a = BREF._checked(labels, action, a256, contour)
    F, H, W = lab.shape
    ch, cw = (H + 1) // 2, (W + 1) // 2
    ry, rc = np.asarray(ys).astype(np.int64) & 0xFFFF, np.asarray(cs).astype(np.int64) & 0xFFFF
    assert ry.shape == (F, H, W) and rc.shape == (F, ch, 2 * cw)
    pal = np.asarray(pal_yuv).astype(np.int64)
    edge = YREF.edges(lab, contour)
    sh = 6 if p010 else 0

    def px(s, p, blurred):
        return np.where(a == 0, s, np.where(a == 3, blurred, np.where(edge, p, (s * (256 - a256) + p * a256 + 128) >> 8)))

    def at_pixels(t):                                # a chroma-plane quantity [F, ch, cw] at the pixels of its 2 x 2 block
        return np.repeat(np.repeat(t, 2, axis=1), 2, axis=2)[:, :H, :W]

    def per_block(t):                                # [F, H, W] -> the sum over the in-picture pixels of every 2 x 2 block
        full = np.zeros((F, 2 * ch, 2 * cw), dtype=np.int64)
        full[:, :H, :W] = t
        return full[:, 0::2, 0::2] + full[:, 0::2, 1::2] + full[:, 1::2, 0::2] + full[:, 1::2, 1::2]
    Y = ry >> sh
    oy = np.where(a == 0, ry, px(Y, pal[lab, 0], within_fn(Y, a == 3, taps)) << sh)
    C = (rc >> sh).reshape(F, ch, cw, 2)
    pair = per_block(a == 3) > 0                     # a pair is a member when any in-picture pixel of its block has action 3
    withinC = within_fn(C, pair, taps_c)             # the chroma plane's own grid of pairs, U and V separately
    n = per_block(np.ones((F, H, W), dtype=np.int64))                 # 1, 2 or 4
    log2n = n >> 1                                                    # 0, 1, 2
    kept = per_block(a != 0) == 0                                     # every in-picture pixel of the block is kept
    oc = rc.reshape(F, ch, cw, 2).copy()
    for k in (0, 1):
        total = per_block(px(at_pixels(C[..., k]), pal[lab, 1 + k], at_pixels(withinC[..., k])))
        oc[..., k] = np.where(kept, oc[..., k], ((total + n // 2) >> log2n) << sh)
    dt = np.uint16 if p010 else np.uint8
    return oy.astype(dt), oc.reshape(F, ch, 2 * cw).astype(dt)
