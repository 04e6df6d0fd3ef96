"""A sequential tracer of the outline rule of include/mdqe_hip.h (mdqe_label_polygons_u8), for the tests: build the directed edge set
of a region, follow the successors, keep the corners, rotate each ring to its smallest key, sort the rings by key.  Plain Python and
numpy, one edge at a time; it shares no code with mdqe_cvpr2023_amd/polygons.py."""
import numpy as np

E, S, W, N = 0, 1, 2, 3
STEP = {E: (1, 0), S: (0, 1), W: (-1, 0), N: (0, -1)}             # (dX, dY); Y goes down


def region_edges(mask):
    """The directed unit edges of a bool region [H, W], the region on the right: {(X, Y, heading)} keyed by the tail vertex."""
    H, Wd = mask.shape
    inside = lambda x, y: 0 <= x < Wd and 0 <= y < H and bool(mask[y, x])
    edges = set()
    for y in range(H):
        for x in range(Wd):
            if not mask[y, x]:
                continue
            if not inside(x, y - 1):
                edges.add((x, y, E))
            if not inside(x + 1, y):
                edges.add((x + 1, y, S))
            if not inside(x, y + 1):
                edges.add((x + 1, y + 1, W))
            if not inside(x - 1, y):
                edges.add((x, y + 1, N))
    return edges


def successor(edges, edge):
    x, y, h = edge
    dx, dy = STEP[h]
    hx, hy = x + dx, y + dy
    for turn in (1, 0, 3):                                          # right, straight on, left
        cand = (hx, hy, (h + turn) % 4)
        if cand in edges:
            return cand
    raise AssertionError("an edge without a successor: %r" % (edge,))


def region_rings(mask):
    """The rings of one region: a list of (start key (Y, X, heading), [(X, Y), ...] corners from the start along the successors)."""
    edges = region_edges(mask)
    left, rings = set(edges), []
    while left:
        first = min(left)
        ring, e = [], first
        while True:
            ring.append(e)
            left.discard(e)
            e = successor(edges, e)
            if e == first:
                break
        corners = [ring[i] for i in range(len(ring)) if ring[i - 1][2] != ring[i][2]]
        keys = [(y, x, h) for x, y, h in corners]
        at = keys.index(min(keys))
        corners = corners[at:] + corners[:at]
        rings.append((keys[at], [(x, y) for x, y, _ in corners]))
    return rings


def trace(labels, n, min_area=0):
    """labels uint8 [F, H, W] -> (xy int32 [V, 2], rings int32 [R, 5]) by the rule: rows k = 0..n-1 (label k + 1), regions of fewer
    than max(1, min_area) pixels left out, rings by ascending (f, Y, X, heading) of their start."""
    labels = np.asarray(labels)
    found = []
    for f in range(labels.shape[0]):
        for k in range(n):
            mask = labels[f] == k + 1
            if int(mask.sum()) < max(1, int(min_area)):
                continue
            for key, pts in region_rings(mask):
                found.append(((f,) + key, k, pts))
    found.sort(key=lambda r: r[0])
    xy, rings = [], []
    for key, k, pts in found:
        rings.append((k, key[0], len(xy), len(pts), 1 if key[3] == S else 0))
        xy.extend(pts)
    return (np.asarray(xy, dtype=np.int32).reshape(-1, 2), np.asarray(rings, dtype=np.int32).reshape(-1, 5))


def area2(pts):
    """sum(x_i * y_{i+1} - x_{i+1} * y_i) over a ring, in Python integers."""
    return sum(int(pts[i][0]) * int(pts[(i + 1) % len(pts)][1]) - int(pts[(i + 1) % len(pts)][0]) * int(pts[i][1]) for i in range(len(pts)))
