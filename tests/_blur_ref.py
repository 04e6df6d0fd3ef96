"""The rule of mdqe_render_blur_u8 and mdqe_render_blur_yuv420sp (include/mdqe_hip.h) restated in numpy int64: the oracle of the blur
tests.  Written from the header's text; it shares nothing with the package's torch host path.  The source values and the edges are those
of tests/_overlay_ref.py / tests/_overlay_yuv_ref.py (the header defines them by reference to the plain overlay's).  The blur is
vectorised by shifted sums over an edge-padded copy (`blur`); `blur_loops` is the same rule as plain loops per pixel, the way it is
written down, which `blur` is checked against on a small case.  Integers only, so every comparison against it is exact."""
import numpy as np

import _overlay_ref as OREF
import _overlay_yuv_ref as YREF


def _taps(taps):
    w = [int(v) for v in np.asarray(taps).astype(np.int64) & 0xFFFF]
    assert 1 <= len(w) <= 33 and w[0] + 2 * sum(w[1:]) == 4096, w
    return w, len(w) - 1


def blur(v, taps):
    """v int64 [F, h, w(, C)] -> same shape: rows first, (sum + 128) >> 8, then columns, (sum + 32768) >> 16, the border replicated."""
    w, R = _taps(taps)
    v = np.asarray(v).astype(np.int64)

    def one(t, axis, add, shift):
        n = t.shape[axis]
        pad = [(0, 0)] * t.ndim
        pad[axis] = (R, R)
        e = np.pad(t, pad, mode="edge")
        acc = np.zeros_like(t)
        for d in range(-R, R + 1):
            acc += w[abs(d)] * np.take(e, np.arange(R + d, R + d + n), axis=axis)
        return (acc + add) >> shift
    return one(one(v, 2, 128, 8), 1, 32768, 16)


def blur_loops(v, taps):
    """`blur` as loops over the pixels and the taps, with the clamped coordinates of the header."""
    w, R = _taps(taps)
    v = np.asarray(v).astype(np.int64)
    F, H, W = v.shape[:3]
    h = np.zeros_like(v)
    out = np.zeros_like(v)
    for Y in range(H):
        for X in range(W):
            acc = 0
            for d in range(-R, R + 1):
                acc = acc + w[abs(d)] * v[:, Y, min(max(X + d, 0), W - 1)]
            h[:, Y, X] = (acc + 128) >> 8
    assert h.max(initial=0) <= 16368
    for Y in range(H):
        for X in range(W):
            acc = 0
            for d in range(-R, R + 1):
                acc = acc + w[abs(d)] * h[:, min(max(Y + d, 0), H - 1), X]
            assert np.max(acc) < 2 ** 26
            out[:, Y, X] = (acc + 32768) >> 16
    return out


def _checked(labels, action, a256, contour):
    lab, act = np.asarray(labels), np.asarray(action)
    assert lab.dtype == np.uint8 and lab.ndim == 3 and act.shape == (256,)
    assert 0 <= a256 <= 256 and 0 <= contour <= 3
    a = act.astype(np.int64)[lab]
    return lab, np.where((a == 1) | (a == 3), a, 0)                   # any other value acts as 0


def paint(labels, frames, palette, action, a256=128, contour=1, taps=(4096,), blur_fn=blur):
    """RGB -> uint8 [F, Ho, Wo, 3].  labels uint8 [F, Ho, Wo]; frames [F, 3, h0, w0] uint8 / float32 or None; palette uint8 [256, 3];
    action [256] of 0 keep / 1 tint / 3 blur; taps [R + 1]."""
    lab, a = _checked(labels, action, a256, contour)
    F, Ho, Wo = lab.shape
    s = OREF.source_values(frames, F, Ho, Wo)
    col = np.asarray(palette).astype(np.int64)[lab]
    tinted = np.where(OREF.edges(lab, contour)[..., None], col, (s * (256 - a256) + col * a256 + 128) >> 8)
    out = np.where((a == 0)[..., None], s, np.where((a == 3)[..., None], blur_fn(s, taps), tinted))
    return out.astype(np.uint8)


def paint_yuv(ys, cs, labels, pal_yuv, action, fmt, a256=128, contour=1, taps=(4096,), taps_c=(4096,), blur_fn=blur):
    """Stored samples in, stored samples out, as _overlay_yuv_ref.paint: ys [F, H, W], cs [F, ceil(H/2), 2*ceil(W/2)], labels uint8
    [F, H, W], pal_yuv [256, 3] -> (ys', cs')."""
    p010 = fmt == "p010"
    lab, a = _checked(labels, action, a256, contour)
    F, H, W = lab.shape
    ch, cw = (H + 1) // 2, (W + 1) // 2
    ry, rc = np.asarray(ys).astype(np.int64) & 0xFFFF, np.asarray(cs).astype(np.int64) & 0xFFFF
    assert ry.shape == (F, H, W) and rc.shape == (F, ch, 2 * cw)
    pal = np.asarray(pal_yuv).astype(np.int64)
    edge = YREF.edges(lab, contour)
    sh = 6 if p010 else 0

    def px(s, p, blurred):
        return np.where(a == 0, s, np.where(a == 3, blurred, np.where(edge, p, (s * (256 - a256) + p * a256 + 128) >> 8)))
    Y = ry >> sh
    oy = np.where(a == 0, ry, px(Y, pal[lab, 0], blur_fn(Y, taps)) << sh)
    C = (rc >> sh).reshape(F, ch, cw, 2)
    blurC = blur_fn(C, taps_c)                       # the chroma plane's own grid of pairs, U and V separately

    def at_pixels(t):                                # a chroma-plane quantity [F, ch, cw] at the pixels of its 2 x 2 block
        return np.repeat(np.repeat(t, 2, axis=1), 2, axis=2)[:, :H, :W]

    def per_block(t):                                # [F, H, W] -> the sum over the in-picture pixels of every 2 x 2 block
        full = np.zeros((F, 2 * ch, 2 * cw), dtype=np.int64)
        full[:, :H, :W] = t
        return full[:, 0::2, 0::2] + full[:, 0::2, 1::2] + full[:, 1::2, 0::2] + full[:, 1::2, 1::2]
    n = per_block(np.ones((F, H, W), dtype=np.int64))                 # 1, 2 or 4
    log2n = n >> 1                                                    # 0, 1, 2
    kept = per_block(a != 0) == 0                                     # every in-picture pixel of the block is kept
    oc = rc.reshape(F, ch, cw, 2).copy()
    for k in (0, 1):
        total = per_block(px(at_pixels(C[..., k]), pal[lab, 1 + k], at_pixels(blurC[..., k])))
        oc[..., k] = np.where(kept, oc[..., k], ((total + n // 2) >> log2n) << sh)
    dt = np.uint16 if p010 else np.uint8
    return oy.astype(dt), oc.reshape(F, ch, 2 * cw).astype(dt)


def action_tables(seed=0):
    """The tables of the tests: every label blurred, the background only, a random mix of 0 / 1 / 3, and the plain overlay's."""
    rng = np.random.default_rng(seed)
    plain = np.ones(256, dtype=np.uint8)
    plain[0] = 0
    bg = plain.copy()
    bg[0] = 3
    return {"all": np.full(256, 3, dtype=np.uint8), "background": bg,
            "mix": np.array([0, 1, 3], dtype=np.uint8)[rng.integers(0, 3, size=256)], "plain": plain}
