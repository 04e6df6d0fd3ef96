"""The track paths' rule (include/mdqe_hip.h, mdqe_label_centroids_u8 / mdqe_render_trails_u8 / mdqe_render_trails_yuv420sp) restated
from its text: centroids as sums over boolean masks turned into Python integers, trails as a PAINTER'S ALGORITHM -- per frame the labels
in descending order, each stroke's hit mask evaluated with the rule's three cases over every pixel it can reach, so whatever is painted
last wins, which is "the first label in ascending order" said the other way round.  Nothing here compacts lists or walks tiles.  Pictures
and surfaces are given as numpy arrays and returned as copies."""
import numpy as np


def centroids(labels, n, min_area=0):
    """labels uint8 [F, Ho, Wo] -> (mom int64 [n, F, 3] = (m, SX, SY), pts int32 [n, F, 2] = (cx, cy), (-1, -1) where absent)."""
    F, Ho, Wo = labels.shape
    mom = np.zeros((n, F, 3), dtype=np.int64)
    pts = np.full((n, F, 2), -1, dtype=np.int32)
    for k in range(n):
        for f in range(F):
            ys, xs = np.nonzero(labels[f] == k + 1)
            m, sx, sy = len(xs), sum(int(v) for v in xs), sum(int(v) for v in ys)
            mom[k, f] = (m, sx, sy)
            if m >= max(1, min_area):
                pts[k, f] = ((sx + m // 2) // m, (sy + m // 2) // m)
    return mom, pts


def present_points(row, j0, j1, Ho, Wo):
    """The present points of a table row (a sequence of (x, y)) in columns j0..j1, in column order, as Python ints."""
    out = []
    for j in range(j0, j1 + 1):
        if j < 0:
            continue
        x, y = int(row[j][0]), int(row[j][1])
        if x < 0 or y < 0 or x >= Wo or y >= Ho:
            continue
        out.append((x, y))
    return out


def strokes_of(points):
    """Each present point gives (P, P); each pair of neighbours in the list of present points (no present point between them) (A, B)."""
    return [(p, p) for p in points] + list(zip(points[:-1], points[1:]))


def stroke_mask(Ho, Wo, A, B, width):
    """(rows, columns, bool mask): the pixels the stroke (A, B) hits, evaluated over the stroke's box grown by `width` and clipped to
    the picture -- a hit pixel lies within width / 2 of the segment, so none is outside it.  int64 throughout: coordinates are below
    2^14, 4*c*c below 2^61."""
    ys = slice(max(min(A[1], B[1]) - width, 0), min(max(A[1], B[1]) + width + 1, Ho))
    xs = slice(max(min(A[0], B[0]) - width, 0), min(max(A[0], B[0]) + width + 1, Wo))
    Y, X = np.mgrid[ys, xs].astype(np.int64)
    dx, dy = B[0] - A[0], B[1] - A[1]
    px, py = X - A[0], Y - A[1]
    L2 = dx * dx + dy * dy
    s = px * dx + py * dy
    w2 = width * width
    qx, qy = X - B[0], Y - B[1]
    c = px * dy - py * dx
    near_a = 4 * (px * px + py * py) <= w2
    near_b = 4 * (qx * qx + qy * qy) <= w2
    side = 4 * c * c <= w2 * L2
    if L2 == 0:
        return ys, xs, near_a
    return ys, xs, np.where(s <= 0, near_a, np.where(s >= L2, near_b, side))


def layer(pts, n, f, p_off, trail, width, Ho, Wo, palette):
    """One frame -> (hit bool [Ho, Wo], col int64 [Ho, Wo, 3]): which pixels the pass writes and with what."""
    hit = np.zeros((Ho, Wo), dtype=bool)
    col = np.zeros((Ho, Wo, 3), dtype=np.int64)
    pal = np.asarray(palette).astype(np.int64)
    for k in reversed(range(n)):
        points = present_points(pts[k], p_off + f - trail, p_off + f, Ho, Wo)
        for A, B in strokes_of(points):
            ys, xs, m = stroke_mask(Ho, Wo, A, B, width)
            hit[ys, xs] |= m
            col[ys, xs][m] = pal[k + 1]
    return hit, col


def trails_rgb(pic, pts, n, palette, F, f_off=0, p_off=0, trail=16, width=2):
    """pic uint8 [N, Ho, Wo, 3]; pts int [>= n, >= p_off + F, 2] -> the painted copy (frames f_off .. f_off + F - 1 drawn on)."""
    out = pic.copy()
    Ho, Wo = pic.shape[1:3]
    for f in range(F):
        hit, col = layer(pts, n, f, p_off, trail, width, Ho, Wo, palette)
        out[f_off + f][hit] = col[hit].astype(np.uint8)
    return out


def paint_yuv(luma, chroma, hit, col, fmt, H, W):
    """The surface form of "write the hit pixels", in place on one surface's STORED planes (bytes for "nv12", 16-bit words for "p010",
    padding and all).  Luma: per sample.  A chroma pair with a hit in its in-picture 2 x 2 block: (sum + n / 2) >> log2(n) over the
    block's n in-picture pixels of the hit's component or the stored sample's value, written as value << 6 for P010; every other
    sample keeps its stored bits."""
    sh = 6 if fmt == "p010" else 0
    CH, CW = (H + 1) // 2, (W + 1) // 2
    inpic = np.zeros((2 * CH, 2 * CW), dtype=bool)
    inpic[:H, :W] = True
    in4 = inpic.reshape(CH, 2, CW, 2)
    half = in4.sum((1, 3)) >> 1                                       # n = 1, 2, 4: n / 2 = log2(n) = 0, 1, 2
    luma[:H, :W][hit] = (col[..., 0][hit] << sh).astype(luma.dtype)
    hp = np.zeros_like(inpic)
    hp[:H, :W] = hit
    h4 = hp.reshape(CH, 2, CW, 2)
    touched = h4.any((1, 3))
    for k in (1, 2):
        cp = np.zeros((2 * CH, 2 * CW), dtype=np.int64)
        cp[:H, :W] = col[..., k]
        plane = chroma[:CH, k - 1:2 * CW:2]                           # (a view: U or V of every pair)
        stored = plane.astype(np.int64) >> sh
        vals = np.where(h4, cp.reshape(CH, 2, CW, 2), stored[:, None, :, None])
        s = (vals * in4).sum((1, 3))
        plane[touched] = (((s + half) >> half) << sh)[touched].astype(plane.dtype)


def trails_yuv(y, uv, fmt, H, W, pts, n, palette_yuv, F, f_off=0, p_off=0, trail=16, width=2):
    """y [N, >= H, >= W], uv [N, >= ceil(H/2), >= 2 ceil(W/2)]: the stored samples -> the painted copies."""
    oy, ouv = y.copy(), uv.copy()
    for f in range(F):
        hit, col = layer(pts, n, f, p_off, trail, width, H, W, palette_yuv)
        paint_yuv(oy[f_off + f], ouv[f_off + f], hit, col, fmt, H, W)
    return oy, ouv
