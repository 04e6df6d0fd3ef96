"""The painting rule of mdqe_render_overlay_u8 (include/mdqe_hip.h) restated in numpy: the oracle of the overlay tests.  Integers only, so
every comparison with the device is exact."""
import numpy as np


def source_values(frames, F, Ho, Wo):
    """s [F, Ho, Wo, 3] int64: frames [F, 3, h0, w0] (uint8 or float32, numpy) nearest-sampled at sy = (Y*h0)//Ho, sx = (X*w0)//Wo;
    float32 -> min(max(rint(v), 0), 255) with round-half-even (np.rint), NaN -> 0; no frames: zeros."""
    if frames is None:
        return np.zeros((F, Ho, Wo, 3), dtype=np.int64)
    fr = np.asarray(frames)
    assert fr.shape[0] == F and fr.shape[1] == 3
    h0, w0 = fr.shape[2], fr.shape[3]
    sy = (np.arange(Ho, dtype=np.int64) * h0) // Ho
    sx = (np.arange(Wo, dtype=np.int64) * w0) // Wo
    s = fr[:, :, sy][:, :, :, sx]                                     # [F, 3, Ho, Wo]
    if s.dtype != np.uint8:
        with np.errstate(invalid="ignore"):
            s = np.where(np.isnan(s), 0.0, np.minimum(np.maximum(np.rint(s.astype(np.float32)), 0.0), 255.0))
    return np.ascontiguousarray(np.moveaxis(s, 1, -1)).astype(np.int64)


def edges(labels, r):
    """bool [F, Ho, Wo]: some neighbour at (+-d, 0) or (0, +-d), 1 <= d <= r, lies inside the image and has another label.  (The caller
    applies it to labelled pixels only.)"""
    lab = np.asarray(labels)
    e = np.zeros(lab.shape, dtype=bool)
    for d in range(1, r + 1):
        if d < lab.shape[1]:
            e[:, d:, :] |= lab[:, d:, :] != lab[:, :-d, :]              # the neighbour d rows up
            e[:, :-d, :] |= lab[:, :-d, :] != lab[:, d:, :]             # d rows down
        if d < lab.shape[2]:
            e[:, :, d:] |= lab[:, :, d:] != lab[:, :, :-d]              # d columns left
            e[:, :, :-d] |= lab[:, :, :-d] != lab[:, :, d:]             # d columns right
    return e


def paint(labels, frames, palette, a256=128, contour=1):
    """-> uint8 [F, Ho, Wo, 3] (numpy).  labels uint8 [F, Ho, Wo]; frames [F, 3, h0, w0] uint8 / float32 or None; palette uint8 [256, 3]."""
    lab = np.asarray(labels)
    assert lab.dtype == np.uint8 and lab.ndim == 3 and 0 <= a256 <= 256 and 0 <= contour <= 3
    F, Ho, Wo = lab.shape
    s = source_values(frames, F, Ho, Wo)
    col = np.asarray(palette).astype(np.int64)[lab]                   # [F, Ho, Wo, 3]
    blend = (s * (256 - a256) + col * a256 + 128) >> 8
    out = np.where(edges(lab, contour)[..., None], col, blend)
    out = np.where((lab == 0)[..., None], s, out)
    return out.astype(np.uint8)


def paint_pixelwise(labels, frames, palette, a256=128, contour=1):
    """The same rule as three nested loops, the way it is written down: what `paint` is checked against on small cases."""
    lab = np.asarray(labels)
    F, Ho, Wo = lab.shape
    s = source_values(frames, F, Ho, Wo)
    pal = np.asarray(palette).astype(np.int64)
    out = np.zeros((F, Ho, Wo, 3), dtype=np.uint8)
    for f in range(F):
        for Y in range(Ho):
            for X in range(Wo):
                l = int(lab[f, Y, X])
                if l == 0:
                    out[f, Y, X] = s[f, Y, X]
                    continue
                edge = False
                for d in range(1, contour + 1):
                    for yy, xx in ((Y - d, X), (Y + d, X), (Y, X - d), (Y, X + d)):
                        if 0 <= yy < Ho and 0 <= xx < Wo and int(lab[f, yy, xx]) != l:
                            edge = True
                out[f, Y, X] = pal[l] if edge else (s[f, Y, X] * (256 - a256) + pal[l] * a256 + 128) >> 8
    return out
