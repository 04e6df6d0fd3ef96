"""The rule of mdqe_track_crops_u8 / mdqe_track_crops_yuv420sp (include/mdqe_hip.h) restated in plain numpy loops: the oracle of the
crop tests.  Written from the header's text, pixel by pixel, with Python integers; nothing is vectorised beyond a footprint's sum, so
there is no split to get wrong.  Integers only: every comparison against it is exact.  The per-sample YUV conversion is the rule of
tests/_yuv_ref.py (`rule`), applied to the one sample a source pixel names."""
import numpy as np

import _yuv_ref as YREF

DEAD = (0, 0, -1, -1)


def live(row, Ho, Wo, min_area):
    area, x0, y0, x1, y1 = (int(v) for v in row)
    return area >= max(1, min_area) and 0 <= x0 <= x1 < Wo and 0 <= y0 <= y1 < Ho


def rect_of(row, Ho, Wo, pad256):
    """(X0, Y0, X1, Y1) of a live row."""
    _, x0, y0, x1, y1 = (int(v) for v in row)
    px = ((x1 - x0 + 1) * pad256 + 128) >> 8
    py = ((y1 - y0 + 1) * pad256 + 128) >> 8
    return max(x0 - px, 0), max(y0 - py, 0), min(x1 + px, Wo - 1), min(y1 + py, Ho - 1)


def span(i, length, S, lo):
    """[a, b): the footprint of chip index i along an axis of `length` source pixels from `lo`."""
    return lo + (i * length) // S, lo + ((i + 1) * length + S - 1) // S


def to_u8(frames):
    """The source value of a frame tensor [F, 3, h0, w0]: uint8 as it is, float32 as min(max(rint(v), 0), 255) with NaN -> 0."""
    frames = np.asarray(frames)
    if frames.dtype == np.uint8:
        return frames.astype(np.int64)
    r = np.rint(frames.astype(np.float64))
    return np.where(np.isnan(r), 0, np.clip(r, 0, 255)).astype(np.int64)


def yuv_source(ys, cs, fmt, matrix, full_range, order):
    """sample(f, sy, sx) -> (c0, c1, c2) of surfaces ys [F, H, W], cs [F, ceil(H/2), 2*ceil(W/2)] (samples as stored)."""
    bits = 8 if fmt == "nv12" else 10

    def value(v):
        return int(v) if fmt == "nv12" else (int(v) & 0xFFFF) >> 6

    def sample(f, sy, sx):
        Y, U, V = value(ys[f, sy, sx]), value(cs[f, sy >> 1, 2 * (sx >> 1)]), value(cs[f, sy >> 1, 2 * (sx >> 1) + 1])
        (R, G, B), _ = YREF.rule(Y, U, V, matrix, full_range, bits)
        return (int(R), int(G), int(B)) if order == "rgb" else (int(B), int(G), int(R))
    return sample


def rgb_source(frames):
    s = to_u8(frames)

    def sample(f, sy, sx):
        return int(s[f, 0, sy, sx]), int(s[f, 1, sy, sx]), int(s[f, 2, sy, sx])
    return sample


def crops(sample, h0, w0, labels, geom, n, size, first=0, step=1, pad256=0, min_area=0, cutout=False, fill=(0, 0, 0)):
    """-> (chips uint8 [n, Fc, Sh, Sw, 3], rects int32 [n, Fc, 4]) for the window frames first, first + step, ... < F."""
    labels = np.asarray(labels)
    F, Ho, Wo = labels.shape
    geom = np.asarray(geom).reshape(n, F, 5) if n else np.zeros((0, F, 5), dtype=np.int32)
    Sh, Sw = size
    taken = list(range(first, F, step))
    out = np.zeros((n, len(taken), Sh, Sw, 3), dtype=np.uint8)
    rects = np.zeros((n, len(taken), 4), dtype=np.int32)
    for k in range(n):
        for t, f in enumerate(taken):
            row = geom[k, f]
            if not live(row, Ho, Wo, min_area):
                out[k, t] = fill
                rects[k, t] = DEAD
                continue
            X0, Y0, X1, Y1 = rect_of(row, Ho, Wo, pad256)
            rects[k, t] = (X0, Y0, X1, Y1)
            cw, ch = X1 - X0 + 1, Y1 - Y0 + 1
            for i in range(Sh):
                Ya, Yb = span(i, ch, Sh, Y0)
                for j in range(Sw):
                    Xa, Xb = span(j, cw, Sw, X0)
                    m, sums = 0, [0, 0, 0]
                    for Y in range(Ya, Yb):
                        for X in range(Xa, Xb):
                            if cutout and int(labels[f, Y, X]) != k + 1:
                                continue
                            px = sample(f, (Y * h0) // Ho, (X * w0) // Wo)
                            m += 1
                            for c in range(3):
                                sums[c] += px[c]
                    out[k, t, i, j] = fill if m == 0 else [(sums[c] + m // 2) // m for c in range(3)]
    return out, rects


def crops_fast(src, labels, geom, n, size, first=0, step=1, pad256=0, min_area=0, cutout=False, fill=(0, 0, 0)):
    """`crops` for a source already expanded to the output grid, src int64 [F, Ho, Wo, 3] (the source value of every output pixel):
    the same loops over chip pixels with a footprint's sum taken by numpy.  For the shapes where the per-sample loop would take minutes;
    tests/test_crops_cpu.py holds it to `crops`."""
    labels = np.asarray(labels)
    F, Ho, Wo = labels.shape
    geom = np.asarray(geom).reshape(n, F, 5) if n else np.zeros((0, F, 5), dtype=np.int32)
    Sh, Sw = size
    taken = list(range(first, F, step))
    out = np.zeros((n, len(taken), Sh, Sw, 3), dtype=np.uint8)
    rects = np.zeros((n, len(taken), 4), dtype=np.int32)
    for k in range(n):
        for t, f in enumerate(taken):
            row = geom[k, f]
            if not live(row, Ho, Wo, min_area):
                out[k, t] = fill
                rects[k, t] = DEAD
                continue
            X0, Y0, X1, Y1 = rect_of(row, Ho, Wo, pad256)
            rects[k, t] = (X0, Y0, X1, Y1)
            cw, ch = X1 - X0 + 1, Y1 - Y0 + 1
            own = labels[f] == k + 1
            for i in range(Sh):
                Ya, Yb = span(i, ch, Sh, Y0)
                for j in range(Sw):
                    Xa, Xb = span(j, cw, Sw, X0)
                    block = src[f, Ya:Yb, Xa:Xb].reshape(-1, 3)
                    if cutout:
                        block = block[own[Ya:Yb, Xa:Xb].reshape(-1)]
                    m = int(block.shape[0])
                    out[k, t, i, j] = fill if m == 0 else [(int(v) + m // 2) // m for v in block.sum(0)]
    return out, rects


def expand_rgb(frames, Ho, Wo):
    """The source value of every output pixel: int64 [F, Ho, Wo, 3] from frames [F, 3, h0, w0]."""
    s = to_u8(frames)
    h0, w0 = s.shape[2:]
    sy, sx = (np.arange(Ho) * h0) // Ho, (np.arange(Wo) * w0) // Wo
    return np.moveaxis(s[:, :, sy][:, :, :, sx], 1, -1)


def expand_yuv(ys, cs, H, W, fmt, matrix, full_range, order, Ho, Wo):
    """The same from surfaces, through tests/_yuv_ref.py's conversion of the whole picture."""
    return expand_rgb(YREF.convert(ys, cs, H, W, fmt, matrix, full_range, order), Ho, Wo)


def box_of(mask):
    """(area, xmin, ymin, xmax, ymax) of a bool [Ho, Wo] plane, the empty row of mdqe_final_masks_u8_geom for an empty one."""
    Ho, Wo = mask.shape
    ys, xs = np.nonzero(mask)
    if not len(ys):
        return (0, Wo, Ho, -1, -1)
    return (int(len(ys)), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
