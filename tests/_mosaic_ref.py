"""The rule of mdqe_render_mosaic_u8 and mdqe_render_mosaic_yuv420sp (include/mdqe_hip.h) restated in numpy int64 with explicit loops over
the cells: the oracle of the mosaic tests.  Written from the header's text; it shares nothing with the package's torch host path.  The
source values and the edges are those of tests/_overlay_ref.py / tests/_overlay_yuv_ref.py (the header defines them by reference to the
plain overlay's).  Integers only, so every comparison against it is exact."""
import numpy as np

import _overlay_ref as OREF
import _overlay_yuv_ref as YREF


def cell_means(v, cell):
    """v int64 [F, h, w(, C)] -> same shape: every position replaced by (sum + n // 2) // n over the n in-picture positions of its
    cell x cell square, squares anchored at (0, 0)."""
    out = np.empty_like(v)
    h, w = v.shape[1], v.shape[2]
    for y0 in range(0, h, cell):
        for x0 in range(0, w, cell):
            blk = v[:, y0:y0 + cell, x0:x0 + cell]
            n = blk.shape[1] * blk.shape[2]
            out[:, y0:y0 + cell, x0:x0 + cell] = ((blk.sum(axis=(1, 2), keepdims=True) + n // 2) // n)
    return out


def _checked(labels, action, a256, contour, cell):
    lab, act = np.asarray(labels), np.asarray(action)
    assert lab.dtype == np.uint8 and lab.ndim == 3 and act.shape == (256,) and set(np.unique(act)) <= {0, 1, 2}
    assert 0 <= a256 <= 256 and 0 <= contour <= 3 and cell % 2 == 0 and 2 <= cell <= 64
    return lab, act.astype(np.int64)[lab]


def paint(labels, frames, palette, action, a256=128, contour=1, cell=16):
    """RGB -> uint8 [F, Ho, Wo, 3].  labels uint8 [F, Ho, Wo]; frames [F, 3, h0, w0] uint8 / float32 or None; palette uint8 [256, 3];
    action [256] of 0 keep / 1 tint / 2 mosaic."""
    lab, a = _checked(labels, action, a256, contour, cell)
    F, Ho, Wo = lab.shape
    s = OREF.source_values(frames, F, Ho, Wo)
    col = np.asarray(palette).astype(np.int64)[lab]
    tinted = np.where(OREF.edges(lab, contour)[..., None], col, (s * (256 - a256) + col * a256 + 128) >> 8)
    out = np.where((a == 0)[..., None], s, np.where((a == 2)[..., None], cell_means(s, cell), tinted))
    return out.astype(np.uint8)


def paint_yuv(ys, cs, labels, pal_yuv, action, fmt, a256=128, contour=1, cell=16):
    """Stored samples in, stored samples out, as _overlay_yuv_ref.paint: ys [F, H, W], cs [F, ceil(H/2), 2*ceil(W/2)], labels uint8
    [F, H, W], pal_yuv [256, 3] -> (ys', cs')."""
    p010 = fmt == "p010"
    lab, a = _checked(labels, action, a256, contour, cell)
    F, H, W = lab.shape
    ch, cw = (H + 1) // 2, (W + 1) // 2
    ry, rc = np.asarray(ys).astype(np.int64) & 0xFFFF, np.asarray(cs).astype(np.int64) & 0xFFFF
    assert ry.shape == (F, H, W) and rc.shape == (F, ch, 2 * cw)
    pal = np.asarray(pal_yuv).astype(np.int64)
    edge = YREF.edges(lab, contour)
    sh = 6 if p010 else 0

    def px(a_, e_, s, p, mean):                      # whole planes, or one pixel of every frame
        return np.where(a_ == 0, s, np.where(a_ == 2, mean, np.where(e_, p, (s * (256 - a256) + p * a256 + 128) >> 8)))
    Y = ry >> sh
    oy = np.where(a == 0, ry, px(a, edge, Y, pal[lab, 0], cell_means(Y, cell)) << sh)
    C = (rc >> sh).reshape(F, ch, cw, 2)
    meanC = cell_means(C, cell // 2)                 # the chroma plane's own cells of (cell/2) x (cell/2) pairs

    def at_pixels(t):                                # a chroma-plane quantity [F, ch, cw] at the pixels of its 2 x 2 block
        return np.repeat(np.repeat(t, 2, axis=1), 2, axis=2)[:, :H, :W]

    def per_block(t):                                # [F, H, W] -> the sum over the in-picture pixels of every 2 x 2 block
        full = np.zeros((F, 2 * ch, 2 * cw), dtype=np.int64)
        full[:, :H, :W] = t
        return full[:, 0::2, 0::2] + full[:, 0::2, 1::2] + full[:, 1::2, 0::2] + full[:, 1::2, 1::2]
    n = per_block(np.ones((F, H, W), dtype=np.int64))                 # 1, 2 or 4
    log2n = n >> 1                                                    # 0, 1, 2
    kept = per_block(a != 0) == 0                                     # every in-picture label of the block has action 0
    oc = rc.reshape(F, ch, cw, 2).copy()
    for k in (0, 1):
        total = per_block(px(a, edge, at_pixels(C[..., k]), pal[lab, 1 + k], at_pixels(meanC[..., k])))
        oc[..., k] = np.where(kept, oc[..., k], ((total + n // 2) >> log2n) << sh)
    dt = np.uint16 if p010 else np.uint8
    return oy.astype(dt), oc.reshape(F, ch, 2 * cw).astype(dt)


def action_tables(seed=0):
    """The tables of the tests: every label a mosaic, the background only, a random mix of 0 / 1 / 2, and the plain overlay's."""
    rng = np.random.default_rng(seed)
    plain = np.ones(256, dtype=np.uint8)
    plain[0] = 0
    bg = plain.copy()
    bg[0] = 2
    return {"all": np.full(256, 2, dtype=np.uint8), "background": bg, "mix": rng.integers(0, 3, size=256).astype(np.uint8),
            "plain": plain}
