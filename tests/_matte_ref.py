"""The rules of mdqe_final_matte_u8 and mdqe_render_replace_u8 (include/mdqe_hip.h) restated on the CPU: the matte in float64 from the
oracle's up-sampled logits, the compositing painter in numpy int64.  Each in two forms, vectorised and written pixelwise the way the
header says it; test_matte_cpu.py holds them against each other, the GPU tests use the vectorised ones."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _overlay_ref as OREF  # noqa: E402

FACTOR = 4


def oracle_values(lg, h, w, Ho, Wo, factor=FACTOR):
    """mdqe/mdqe.py:357-358 + 458-462 in float64, as test_label_map_gpu._oracle_values does it: x4 aligned bilinear, crop, nearest
    resize of logits [k, Fw, Hm, Wm] -> (values float64 numpy [k, Fw, Ho, Wo], bits = sigmoid(value) > 0.5)."""
    import mdqe_oracle as O
    up = O.aligned_bilinear(lg.double(), factor)[..., :h, :w]
    if up.shape[0] == 0:
        return np.zeros((0, lg.shape[1], Ho, Wo)), np.zeros((0, lg.shape[1], Ho, Wo), dtype=bool)
    v = F.interpolate(up, size=(Ho, Wo), mode="nearest")
    return v.numpy(), (v.sigmoid() > 0.5).numpy()


def participating(rows, take):
    """Which of the selected rows take part: all (take None), else those whose label rows[k] + 1 has a nonzero entry."""
    return [k for k, r in enumerate(rows) if take is None or int(take[r + 1]) != 0]


def matte(v, bits, gain):
    """v float64 [k, Fw, Ho, Wo] and bits bool of the PARTICIPATING rows -> (plane uint8 [Fw, Ho, Wo], the float64 level 255 * p it
    rounds, vmax).  gain: the fp32 value the device multiplies by."""
    if v.shape[0] == 0:
        z = np.zeros(v.shape[1:])
        return z.astype(np.uint8), z, z
    g = float(np.float32(gain))
    vmax, U = v.max(0), bits.any(0)
    level = 255.0 / (1.0 + np.exp(-g * vmax))
    a = np.rint(level).astype(np.int64)
    return np.where(U, np.maximum(a, 128), np.minimum(a, 127)).astype(np.uint8), level, vmax


def matte_pixelwise(v, bits, gain):
    """`matte`'s plane pixel by pixel, the way the header writes it."""
    k, Fw, Ho, Wo = v.shape
    out = np.zeros((Fw, Ho, Wo), dtype=np.uint8)
    g = float(np.float32(gain))
    for f in range(Fw):
        for Y in range(Ho):
            for X in range(Wo):
                if k == 0:
                    continue
                vmax, U = max(float(v[i, f, Y, X]) for i in range(k)), any(bool(bits[i, f, Y, X]) for i in range(k))
                p = 1.0 / (1.0 + np.exp(-g * vmax))
                a = int(np.rint(255.0 * p))
                out[f, Y, X] = max(a, 128) if U else min(a, 127)
    return out


def mix(s, b, w):
    """(s * w + b * (255 - w) + 127) // 255 on int64 arrays (or ints)."""
    return (s * w + b * (255 - w) + 127) // 255


def _base(lab, frames, palette, action, a256, contour):
    """The overlay rule's pixel with the action deciding (1 tints, anything else keeps the source) -> int64 [F, Ho, Wo, 3]."""
    Fn, Ho, Wo = lab.shape
    s = OREF.source_values(frames, Fn, Ho, Wo)
    col = np.asarray(palette).astype(np.int64)[lab]
    tinted = np.where(OREF.edges(lab, contour)[..., None], col, (s * (256 - a256) + col * a256 + 128) >> 8)
    return np.where((np.asarray(action).astype(np.int64)[lab] == 1)[..., None], tinted, s)


def replace_rgb(labels, frames, palette, action, mat, backdrop, a256=128, contour=1, mode=0):
    """-> uint8 [F, Ho, Wo, 3].  labels, mat uint8 [F, Ho, Wo]; frames [F, 3, h0, w0] uint8 / float32 or None; palette uint8 [256, 3];
    action uint8 [256]; backdrop uint8 [3] or [Ho, Wo, 3]; mode 0 background / 1 tracks."""
    lab, m, B = np.asarray(labels), np.asarray(mat).astype(np.int64), np.asarray(backdrop).astype(np.int64)
    assert lab.dtype == np.uint8 and lab.ndim == 3 and m.shape == lab.shape and mode in (0, 1)
    assert B.shape == (3,) or B.shape == lab.shape[1:] + (3,)
    wt = (255 - m if mode else m)[..., None]
    return mix(_base(lab, frames, palette, action, a256, contour), B[None] if B.ndim == 3 else B, wt).astype(np.uint8)


def replace_rgb_pixelwise(labels, frames, palette, action, mat, backdrop, a256=128, contour=1, mode=0):
    """The same rule as nested loops."""
    lab = np.asarray(labels)
    Fn, Ho, Wo = lab.shape
    s = OREF.source_values(frames, Fn, Ho, Wo)
    pal, B = np.asarray(palette).astype(np.int64), np.asarray(backdrop).astype(np.int64)
    out = np.zeros((Fn, Ho, Wo, 3), dtype=np.uint8)
    for f in range(Fn):
        for Y in range(Ho):
            for X in range(Wo):
                l = int(lab[f, Y, X])
                base = [int(c) for c in s[f, Y, X]]
                if int(action[l]) == 1:
                    edge = False
                    for d in range(1, contour + 1):
                        for yy, xx in ((Y - d, X), (Y + d, X), (Y, X - d), (Y, X + d)):
                            if 0 <= yy < Ho and 0 <= xx < Wo and int(lab[f, yy, xx]) != l:
                                edge = True
                    base = [int(pal[l, c]) if edge else (base[c] * (256 - a256) + int(pal[l, c]) * a256 + 128) >> 8 for c in range(3)]
                wt = int(mat[f, Y, X])
                wt = 255 - wt if mode else wt
                back = B[Y, X] if B.ndim == 3 else B
                for c in range(3):
                    out[f, Y, X, c] = (base[c] * wt + int(back[c]) * (255 - wt) + 127) // 255
    return out


def ramp_matte(Fn, Ho, Wo, seed):
    """A matte that holds 0, 255 and everything between: random levels, a run of every level 0..255, and blocks of 0 and of 255."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 256, size=(Fn, Ho, Wo)).astype(np.uint8)
    m[:, : max(1, Ho // 3), : max(1, Wo // 2)] = 255
    m[:, -max(1, Ho // 3):, -max(1, Wo // 2):] = 0
    flat = m.reshape(Fn, -1)
    n = min(256, flat.shape[1])
    flat[0, :n] = np.arange(256, dtype=np.uint8)[:n]                  # (over the first rows of frame 0; the blocks stay whole elsewhere)
    return m


# ---- the surface painter --------------------------------------------------------------------------------------------------------------
def replace_yuv(ys, cs, labels, pal_yuv, action, mat, backdrop, fmt, a256=128, contour=1, mode=0):
    """Stored samples in, stored samples out, as _overlay_yuv_ref.paint: ys [F, H, W], cs [F, ceil(H/2), 2*ceil(W/2)], labels and mat uint8
    [F, H, W], pal_yuv [256, 3]; backdrop: (Y, U, V) in sample units, or (by [H, W], bc [ceil(H/2), 2*ceil(W/2)]) stored samples of one
    surface -> (ys', cs')."""
    import _overlay_yuv_ref as YREF
    p010 = fmt == "p010"
    lab = np.asarray(labels)
    Fn, H, W = lab.shape
    ch, cw = (H + 1) // 2, (W + 1) // 2
    sh = 6 if p010 else 0
    ry, rc = np.asarray(ys).astype(np.int64) & 0xFFFF, np.asarray(cs).astype(np.int64) & 0xFFFF
    assert ry.shape == (Fn, H, W) and rc.shape == (Fn, ch, 2 * cw) and mode in (0, 1)
    pal = np.asarray(pal_yuv).astype(np.int64)
    tinted = np.asarray(action).astype(np.int64)[lab] == 1
    edge = YREF.edges(lab, contour)
    wt = np.asarray(mat).astype(np.int64)
    wt = 255 - wt if mode else wt

    def at_pixels(t):                                # a chroma-plane quantity at the pixels of its 2 x 2 block
        return np.repeat(np.repeat(t, 2, axis=-2), 2, axis=-1)[..., :H, :W]

    def per_block(t):
        full = np.zeros((Fn, 2 * ch, 2 * cw), dtype=np.int64)
        full[:, :H, :W] = t
        return full[:, 0::2, 0::2] + full[:, 0::2, 1::2] + full[:, 1::2, 0::2] + full[:, 1::2, 1::2]
    if isinstance(backdrop, tuple) and len(backdrop) == 2:
        by, bc = ((np.asarray(t).astype(np.int64) & 0xFFFF) >> sh for t in backdrop)
        BY, BC = by[None], [at_pixels(bc.reshape(ch, cw, 2)[..., k])[None] for k in (0, 1)]
    else:
        BY, BC = int(backdrop[0]), [int(backdrop[1]), int(backdrop[2])]

    def base(s, p):
        return np.where(tinted, np.where(edge, p, (s * (256 - a256) + p * a256 + 128) >> 8), s)
    kept = ~tinted & (wt == 255)
    oy = np.where(kept, ry, mix(base(ry >> sh, pal[lab, 0]), BY, wt) << sh)
    C = (rc >> sh).reshape(Fn, ch, cw, 2)
    n = per_block(np.ones((Fn, H, W), dtype=np.int64))
    same = per_block(~kept) == 0
    oc = rc.reshape(Fn, ch, cw, 2).copy()
    for k in (0, 1):
        total = per_block(mix(base(at_pixels(C[..., k]), pal[lab, 1 + k]), BC[k], wt))
        oc[..., k] = np.where(same, oc[..., k], ((total + n // 2) >> (n >> 1)) << sh)
    dt = np.uint16 if p010 else np.uint8
    return oy.astype(dt), oc.reshape(Fn, ch, 2 * cw).astype(dt)


def replace_yuv_pixelwise(ys, cs, labels, pal_yuv, action, mat, backdrop, fmt, a256=128, contour=1, mode=0):
    """The same rule block by block and pixel by pixel, the way the header writes it."""
    p010 = fmt == "p010"
    sh = 6 if p010 else 0
    lab = np.asarray(labels)
    Fn, H, W = lab.shape
    oy, oc = np.asarray(ys).copy(), np.asarray(cs).copy()
    pal = np.asarray(pal_yuv).astype(np.int64)
    surf = isinstance(backdrop, tuple) and len(backdrop) == 2
    for f in range(Fn):
        for br in range((H + 1) // 2):
            for bc in range((W + 1) // 2):
                px = [(r, c) for r in (2 * br, 2 * br + 1) for c in (2 * bc, 2 * bc + 1) if r < H and c < W]
                n, tot, same = len(px), [0, 0], True
                for r, c in px:
                    l = int(lab[f, r, c])
                    tinted = int(action[l]) == 1
                    edge = any(0 <= yy < H and 0 <= xx < W and int(lab[f, yy, xx]) != l
                               for d in range(1, contour + 1) for yy, xx in ((r - d, c), (r + d, c), (r, c - d), (r, c + d)))
                    wt = int(mat[f, r, c])
                    wt = 255 - wt if mode else wt

                    def base(s, p):
                        return (p if edge else (s * (256 - a256) + p * a256 + 128) >> 8) if tinted else s
                    raw = int(ys[f, r, c])
                    BY = (int(backdrop[0][r, c]) >> sh) if surf else int(backdrop[0])
                    if tinted or wt != 255:
                        oy[f, r, c] = mix(base(raw >> sh, int(pal[l, 0])), BY, wt) << sh
                        same = False
                    for k in (0, 1):
                        BC = (int(backdrop[1][br, 2 * bc + k]) >> sh) if surf else int(backdrop[1 + k])
                        tot[k] += mix(base(int(cs[f, br, 2 * bc + k]) >> sh, int(pal[l, 1 + k])), BC, wt)
                if not same:
                    for k in (0, 1):
                        oc[f, br, 2 * bc + k] = ((tot[k] + n // 2) >> {1: 0, 2: 1, 4: 2}[n]) << sh
    return oy, oc
