"""The annotation pass's rule (include/mdqe_hip.h, mdqe_annotate_u8 / mdqe_annotate_yuv420sp) restated in numpy as a PAINTER'S
ALGORITHM: per frame, the box frames are filled in descending label order, then the plates in descending label order, each fill a
slice assignment, so whatever is painted last wins -- which is the kernel's "first hit in ascending order, plates before frames" said
the other way round.  Nothing here walks a list per pixel.  Pictures and surfaces are given as numpy arrays and returned as copies."""
import numpy as np


def is_live(row, Ho, Wo, min_area):
    area, x0, y0, x1, y1 = (int(v) for v in row)
    return area >= max(1, min_area) and 0 <= x0 <= x1 < Wo and 0 <= y0 <= y1 < Ho


def text_of(captions, l):
    """The bytes of caption row l before its first 0 byte."""
    row = bytes(captions[l].tolist())
    return row.split(b"\0")[0]


def plate_of(text, font, scale):
    """-> the ink mask bool [9 * scale, (6c + 1) * scale] of a plate that holds `text` (c >= 1 bytes)."""
    c = len(text)
    small = np.zeros((9, 6 * c + 1), dtype=bool)
    for i, ch in enumerate(text):
        glyph = font[(ch if 0x20 <= ch <= 0x5F else 0x3F) - 32]
        for gy in range(7):
            for x in range(5):
                small[1 + gy, 1 + 6 * i + x] = bool((int(glyph[gy]) >> (4 - x)) & 1)
    return np.repeat(np.repeat(small, scale, axis=0), scale, axis=1)


def layers(geom_f, n, Ho, Wo, palette, ink, captions, font, box, scale, min_area):
    """One frame: geom_f [n, 5] -> (hit bool [Ho, Wo], col int64 [Ho, Wo, 3]): which pixels the pass writes and with what."""
    hit = np.zeros((Ho, Wo), dtype=bool)
    col = np.zeros((Ho, Wo, 3), dtype=np.int64)
    pal, ik = palette.astype(np.int64), ink.astype(np.int64)
    lives = [k + 1 for k in range(n) if is_live(geom_f[k], Ho, Wo, min_area)]
    if box > 0:
        for l in reversed(lives):
            _, x0, y0, x1, y1 = (int(v) for v in geom_f[l - 1])
            bands = ((slice(y0, min(y0 + box, y1 + 1)), slice(x0, x1 + 1)), (slice(max(y1 - box + 1, y0), y1 + 1), slice(x0, x1 + 1)),
                     (slice(y0, y1 + 1), slice(x0, min(x0 + box, x1 + 1))), (slice(y0, y1 + 1), slice(max(x1 - box + 1, x0), x1 + 1)))
            for ys, xs in bands:
                hit[ys, xs] = True
                col[ys, xs] = pal[l]
    if captions is not None:
        for l in reversed(lives):
            text = text_of(captions, l)
            if not text:
                continue
            _, x0, y0, _, _ = (int(v) for v in geom_f[l - 1])
            mask = plate_of(text, font, scale)
            h, w = mask.shape
            px = max(0, min(x0, Wo - w))
            py = y0 - h if y0 - h >= 0 else y0
            part = mask[:Ho - py, :Wo - px]                           # clipped to the picture
            hit[py:py + h, px:px + w] = True
            col[py:py + h, px:px + w] = np.where(part[..., None], ik[l], pal[l])
    return hit, col


def annotate(pic, geom, n, palette, ink, captions, font, f_off=0, box=0, scale=1, min_area=0):
    """pic uint8 [N, Ho, Wo, 3]; geom int [n * F, 5] -> the annotated copy (frames f_off .. f_off + F - 1 drawn on)."""
    out = pic.copy()
    if n == 0:
        return out
    Ho, Wo = pic.shape[1:3]
    g = np.asarray(geom).reshape(n, -1, 5)
    for f in range(g.shape[1]):
        hit, col = layers(g[:, f], n, Ho, Wo, palette, ink, captions, font, box, scale, min_area)
        out[f_off + f][hit] = col[hit].astype(np.uint8)
    return out


def annotate_yuv(y, uv, fmt, H, W, geom, n, palette_yuv, ink_yuv, captions, font, f_off=0, box=0, scale=1, min_area=0):
    """y [N, >= H, >= W], uv [N, >= ceil(H/2), >= 2 ceil(W/2)]: the STORED samples (bytes for "nv12", 16-bit words for "p010", padding
    and all) -> the annotated copies.  Luma: the rule per sample.  A chroma pair with a hit in its in-picture block: (sum + n / 2) >>
    log2(n) over the block's n in-picture pixels of the hit's component or the stored sample's value, written as value << 6 for P010;
    every other sample keeps its stored bits."""
    oy, ouv = y.copy(), uv.copy()
    if n == 0:
        return oy, ouv
    sh = 6 if fmt == "p010" else 0
    CH, CW = (H + 1) // 2, (W + 1) // 2
    g = np.asarray(geom).reshape(n, -1, 5)
    inpic = np.zeros((2 * CH, 2 * CW), dtype=bool)
    inpic[:H, :W] = True
    in4 = inpic.reshape(CH, 2, CW, 2)
    count = in4.sum((1, 3))
    half = count >> 1                                                 # n = 1, 2, 4: n / 2 = log2(n) = 0, 1, 2
    for f in range(g.shape[1]):
        hit, col = layers(g[:, f], n, H, W, palette_yuv, ink_yuv, captions, font, box, scale, min_area)
        luma = oy[f_off + f]
        luma[:H, :W][hit] = (col[..., 0][hit] << sh).astype(luma.dtype)
        hp = np.zeros_like(inpic)
        hp[:H, :W] = hit
        h4 = hp.reshape(CH, 2, CW, 2)
        touched = h4.any((1, 3))
        for k in (1, 2):
            cp = np.zeros((2 * CH, 2 * CW), dtype=np.int64)
            cp[:H, :W] = col[..., k]
            plane = ouv[f_off + f][:CH, k - 1:2 * CW:2]               # (a view: U or V of every pair)
            stored = plane.astype(np.int64) >> sh
            vals = np.where(h4, cp.reshape(CH, 2, CW, 2), stored[:, None, :, None])
            s = (vals * in4).sum((1, 3))
            plane[touched] = (((s + half) >> half) << sh)[touched].astype(plane.dtype)
    return oy, ouv
