"""Track outlines as a video output: the label map's visible regions as polygons (model.polygon_output, online_video(polygons=...)).
`Polygons` is the request, `TrackPolygons` the result (numpy, on the host: a polygon set is a few KB per window), and
`polygons_from_labels` the rule of include/mdqe_hip.h (mdqe_label_polygons_u8) on the host, for the paths without a device window, as
rle.geometry_dense is for geometry.  On the device the rings come from ops.label_polygons (csrc/polygons.hip) through
merge.polygon_rings.  Coordinates are lattice vertices: pixel (x, y) covers the square (x, y)..(x + 1, y + 1), Y goes down."""
import dataclasses

import numpy as np


@dataclasses.dataclass(frozen=True)
class Polygons:
    """Per-track outline polygons as a video output.  min_area: visible regions of fewer pixels have no rings; every >= 1: the video
    frames f with f % every == 0 are taken; classes: None (every track) or a collection of class ids >= 0 (kept as a sorted tuple):
    only the tracks whose window class row has its first maximum in one of them."""
    min_area: int = 0
    every: int = 1
    classes: tuple = None

    def __post_init__(self):
        if isinstance(self.min_area, bool) or not isinstance(self.min_area, int) or not 0 <= self.min_area < 2 ** 31:
            raise ValueError("polygons: min_area must be an int in 0..2^31 - 1, got %r" % (self.min_area,))
        if isinstance(self.every, bool) or not isinstance(self.every, int) or self.every < 1:
            raise ValueError("polygons: every must be an int >= 1, got %r" % (self.every,))
        if self.classes is not None:
            try:
                cls = tuple(self.classes) if not isinstance(self.classes, (str, bytes)) else None
            except TypeError:
                cls = None
            if cls is None or any(isinstance(c, bool) or not isinstance(c, int) or c < 0 for c in cls):
                raise ValueError("polygons: classes must be None or a collection of ints >= 0, got %r" % (self.classes,))
            object.__setattr__(self, "classes", tuple(sorted(set(cls))))

    def rows(self, cls_probs, n):
        """bool [n]: the window's rows whose rings are kept -- all of them without `classes`, else those whose class row (cls_probs
        [n, K], the window's, on the host) has its first maximum in a listed class."""
        keep = np.ones(int(n), dtype=bool)
        if self.classes is None:
            return keep
        if cls_probs is None or getattr(cls_probs, "ndim", 0) != 2:
            raise ValueError("polygons: classes need the window's class rows [n, K], got %r" % type(cls_probs).__name__)
        probs = cls_probs.detach().cpu().numpy() if hasattr(cls_probs, "detach") else np.asarray(cls_probs)
        keep[:] = False
        m = min(int(n), probs.shape[0])
        if m and probs.shape[1]:
            keep[:m] = np.isin(probs[:m].argmax(1), np.asarray(self.classes))
        return keep

    def keep(self, rings, f0, cls_probs, n):
        """bool [R]: the ring records (frames relative to video frame f0) this request keeps: `every` and `classes`."""
        rings = np.asarray(rings).reshape(-1, 5)
        rows = self.rows(cls_probs, n)
        k = rings[:, 0]
        ok = (k >= 0) & (k < len(rows))
        return ok & rows[np.where(ok, k, 0)] & ((rings[:, 1] + int(f0)) % self.every == 0) if len(rows) else np.zeros(len(rings), dtype=bool)


def select_rings(xy, rings, keep):
    """The ring records `keep` (bool [R]) selects, in their order, with xy compacted and the first-vertex offsets renumbered."""
    xy, rings = np.asarray(xy, dtype=np.int32).reshape(-1, 2), np.asarray(rings, dtype=np.int32).reshape(-1, 5)
    keep = np.asarray(keep, dtype=bool)
    if len(keep) and keep.all() and len(xy) == int(rings[:, 3].sum()) and np.array_equal(rings[1:, 2], np.cumsum(rings[:-1, 3])) \
            and int(rings[0, 2]) == 0:                                 # (everything, as it stands)
        return xy.copy(), rings.copy()
    sel = rings[keep]
    if not len(sel):
        return np.zeros((0, 2), dtype=np.int32), np.zeros((0, 5), dtype=np.int32)
    out = sel.copy()
    count = sel[:, 3].astype(np.int64)
    out[:, 2] = np.concatenate([[0], np.cumsum(count[:-1])])
    pick = np.arange(int(count.sum())) + np.repeat(sel[:, 2] - out[:, 2], count)   # each ring's vertices, moved to its new offset
    return np.ascontiguousarray(xy[pick]), out


class TrackPolygons:
    """The outlines of a window's or a video's tracks.  xy: int32 [V, 2], (X, Y) lattice vertices, ring after ring; rings: int32 [R, 5],
    (row k, frame f, first vertex, vertex count, hole 0|1) -- f in VIDEO frames, k the row in the order of "pred_track_ids" (offline)
    or the window's row (online); size = (H, W).  The rings are in ascending (f, Y, X, heading) of their start corner; an outer ring
    keeps its region on the right (A2 > 0 with Y down), a hole runs the other way."""

    def __init__(self, xy, rings, size):
        self.xy = np.ascontiguousarray(np.asarray(xy, dtype=np.int32).reshape(-1, 2))
        self.rings = np.ascontiguousarray(np.asarray(rings, dtype=np.int32).reshape(-1, 5))
        self.size = (int(size[0]), int(size[1]))

    def __len__(self):
        return len(self.rings)

    def __eq__(self, other):
        return (isinstance(other, TrackPolygons) and self.size == other.size and np.array_equal(self.xy, other.xy)
                and np.array_equal(self.rings, other.rings))

    __hash__ = None

    def __repr__(self):
        return "TrackPolygons(%d rings, %d vertices, size=%s)" % (len(self.rings), len(self.xy), self.size)

    def of(self, k, f):
        """The rings of row k in frame f, in ring order: [(vertices int32 [v, 2], hole bool)]."""
        r = self.rings[(self.rings[:, 0] == int(k)) & (self.rings[:, 1] == int(f))]
        return [(self.xy[a:a + c], bool(h)) for _, _, a, c, h in r.tolist()]

    def area2(self, k, f):
        """The summed A2 = sum(x_i * y_{i+1} - x_{i+1} * y_i) of the rings of (k, f): twice the region's pixel count."""
        total = 0
        for pts, _ in self.of(k, f):
            x, y = pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)
            total += int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())
        return total

    def has_holes(self, k, f):
        return any(hole for _, hole in self.of(k, f))

    def to_coco(self, k, f):
        """The outer rings of (k, f) as COCO `segmentation` lists, [x0, y0, x1, y1, ...] floats; holes are dropped (`has_holes` says when)."""
        return [[float(v) for v in pts.reshape(-1)] for pts, hole in self.of(k, f) if not hole]

    def rasterize(self, k, f):
        """bool [H, W]: the even-odd fill of the rings of (k, f) -- the region they were traced from."""
        H, W = self.size
        flips = np.zeros((H, W + 1), dtype=np.uint8)
        for pts, _ in self.of(k, f):
            nxt = np.roll(pts, -1, axis=0)
            for (x0, y0), (x1, y1) in zip(pts.tolist(), nxt.tolist()):
                if x0 == x1 and y0 != y1:                               # a vertical edge flips everything on its right
                    flips[min(y0, y1):max(y0, y1), x0] ^= 1
        return np.bitwise_xor.accumulate(flips, axis=1)[:, :W].astype(bool)

    def renumbered(self, rows=None, f0=0):
        """A copy with frame f -> f + f0 and row k -> rows[k]; the rings of a row that `rows` (a dict, or a list with None / -1 for
        "dropped") does not name are left out."""
        rings = self.rings.copy()
        keep = np.ones(len(rings), dtype=bool)
        if rows is not None:
            table = rows if isinstance(rows, dict) else {k: v for k, v in enumerate(rows) if v is not None and v >= 0}
            new = np.asarray([table.get(int(k), -1) for k in rings[:, 0]], dtype=np.int32).reshape(-1)
            keep = new >= 0
            rings[:, 0] = new
        rings[:, 1] += int(f0)
        return TrackPolygons(*select_rings(self.xy, rings, keep), self.size)

    @classmethod
    def concat(cls, parts, size=None):
        """The windows' polygons joined in the order given (windows in video order keep the ring order: frames ascend)."""
        parts = list(parts)
        if not parts:
            if size is None:
                raise ValueError("TrackPolygons.concat: no parts and no size")
            return cls(np.zeros((0, 2), np.int32), np.zeros((0, 5), np.int32), size)
        size = parts[0].size if size is None else (int(size[0]), int(size[1]))
        if any(p.size != size for p in parts):
            raise ValueError("TrackPolygons.concat: parts of different sizes %s" % sorted({p.size for p in parts} | {size}))
        rings, at = [], 0
        for p in parts:
            r = p.rings.copy()
            r[:, 2] += at
            at += len(p.xy)
            rings.append(r)
        return cls(np.concatenate([p.xy for p in parts]), np.concatenate(rings), size)


def _region_corners(mask):
    """One region (bool [H, W]) -> (corners int [C, 3] rows (Y, X, heading) in key order, succ int [C]: the next corner of each along
    its ring).  Every lattice vertex is classified at once from its 2 x 2 pixels; along a lattice line the run starts and the run ends
    of one heading alternate, so the i-th start meets the i-th end."""
    P = np.pad(np.asarray(mask, dtype=bool), 1)
    a, b, c, d = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]       # pixels NW, NE, SW, SE of every vertex
    leave = [d & ~b, c & ~d, a & ~c, b & ~a]                           # an edge leaves with heading E, S, W, N
    arrive = [c & ~a, a & ~b, b & ~d, d & ~c]                          # ... arrives with it
    cid = np.full((4,) + a.shape, -1, dtype=np.int64)
    corner = np.stack([leave[h] & ~arrive[h] for h in range(4)], axis=-1)   # [H + 1, W + 1, 4]: nonzero() is the key order
    Y, X, Hd = np.nonzero(corner)
    cid[Hd, Y, X] = np.arange(len(Y))
    succ = np.full(len(Y), -1, dtype=np.int64)
    for h in range(4):
        start, end = leave[h] & ~arrive[h], arrive[h] & ~leave[h]
        if h in (0, 2):                                                 # along rows
            sy, sx = np.nonzero(start)
            ey, ex = np.nonzero(end)
        else:                                                           # along columns
            sx, sy = np.nonzero(start.T)
            ex, ey = np.nonzero(end.T)
        right = leave[(h + 1) % 4][ey, ex]
        turn = np.where(right, (h + 1) % 4, (h + 3) % 4)
        succ[cid[h, sy, sx]] = cid[turn, ey, ex]
    return np.stack([Y, X, Hd], axis=1), succ


def polygons_from_labels(label_map, n, min_area=0):
    """The rule of include/mdqe_hip.h (mdqe_label_polygons_u8) on the host: label_map uint8 [F, H, W] (0 = background, label k + 1 =
    row k; numpy or a host tensor), rows k = 0..n-1 -> TrackPolygons with f the map's frame and k the row.  What ops.label_polygons
    gives on the device, ring for ring."""
    lab = label_map.detach().cpu().numpy() if hasattr(label_map, "detach") else np.asarray(label_map)
    if lab.ndim != 3:
        raise ValueError("polygons_from_labels: label_map must be [F, H, W], got shape %s" % (tuple(lab.shape),))
    need, found = max(1, int(min_area)), []
    for f in range(lab.shape[0]):
        present = np.bincount(lab[f].reshape(-1), minlength=256)
        for k in range(min(int(n), 255)):
            if present[k + 1] < need:
                continue
            region = lab[f] == k + 1
            ys, xs = np.flatnonzero(region.any(1)), np.flatnonzero(region.any(0))
            corners, succ = _region_corners(region[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1])   # (its bounding box: the order is kept)
            corners[:, 0] += ys[0]
            corners[:, 1] += xs[0]
            seen = np.zeros(len(corners), dtype=bool)
            nxt = succ.tolist()
            for s in range(len(corners)):                               # ascending: the first corner met of a ring is its smallest
                if seen[s]:
                    continue
                ring, i = [], s
                while not seen[i]:
                    seen[i] = True
                    ring.append(i)
                    i = nxt[i]
                found.append(((f,) + tuple(corners[s].tolist()), k, corners[ring][:, [1, 0]]))
    found.sort(key=lambda r: r[0])
    rings, at = [], 0
    for key, k, pts in found:
        rings.append((k, key[0], at, len(pts), int(key[3] == 1)))
        at += len(pts)
    xy = np.concatenate([r[2] for r in found]) if found else np.zeros((0, 2), np.int32)
    return TrackPolygons(xy, np.asarray(rings, dtype=np.int32).reshape(-1, 5), lab.shape[1:])
