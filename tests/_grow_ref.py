"""The redaction margin's rule (include/mdqe_hip.h, mdqe_grow_labels_u8) restated in numpy int64, two ways: `grow_pixelwise`, the
definition as loops per pixel over the disc, and `grow`, a sweep of shifted arrays over the disc's offsets.  Neither separates the
minimum into a column and a row pass, as the kernel does.  Integers only: every comparison with them is exact."""
import numpy as np

BIG = np.int64(1) << 40                              # "no candidate": above every key d2 * 256 + label


def growing(table):
    """bool [256]: label g grows when g >= 1 and table[g] != 0; entry 0 is ignored."""
    table = np.asarray(table)
    assert table.shape == (256,)
    g = table != 0
    g[0] = False
    return g


def _checked(labels, table, radius):
    labels = np.asarray(labels)
    assert labels.dtype == np.uint8 and labels.ndim == 3 and isinstance(radius, int) and 0 <= radius <= 32
    return labels, growing(table)


def grow_pixelwise(labels, table, radius):
    """The definition: for every pixel whose label does not grow, the smallest (d2, label) over the growing pixels of its frame inside
    the picture with d2 <= radius^2."""
    labels, g = _checked(labels, table, radius)
    F, H, W = labels.shape
    out = labels.copy()
    for f in range(F):
        ys, xs = np.nonzero(g[labels[f]])
        if not len(ys):
            continue
        ls = labels[f][ys, xs].astype(np.int64)
        for Y in range(H):
            for X in range(W):
                if g[labels[f, Y, X]]:
                    continue
                best = None
                for y, x, l in zip(ys.tolist(), xs.tolist(), ls.tolist()):
                    d2 = (Y - y) ** 2 + (X - x) ** 2
                    if d2 <= radius * radius and (best is None or (d2, l) < best):
                        best = (d2, l)
                if best is not None:
                    out[f, Y, X] = best[1]
    return out


def grow(labels, table, radius):
    """The same by a sweep: for every offset (dy, dx) of the disc, the map shifted by it offers the key d2 * 256 + label where the
    shifted pixel lies inside the picture and grows; the smallest key wins."""
    labels, g = _checked(labels, table, radius)
    F, H, W = labels.shape
    lab = labels.astype(np.int64)
    src = np.where(g[labels], lab, 0)                # the label where it grows, else 0
    if not src.any():
        return labels.copy()
    offer = np.where(src != 0, src, BIG)             # what a pixel offers its neighbours: its label, or no candidate
    best = np.full((F, H, W), BIG, dtype=np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            d2 = dy * dy + dx * dx
            if d2 > radius * radius or abs(dy) >= H or abs(dx) >= W:
                continue
            # pixel (Y, X) looks at (Y + dy, X + dx)
            y0, y1 = max(0, -dy), min(H, H - dy)
            x0, x1 = max(0, -dx), min(W, W - dx)
            view = best[:, y0:y1, x0:x1]
            np.minimum(view, offer[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx] + d2 * 256, out=view)      # (BIG + d2 * 256 stays "none")
    out = np.where((src == 0) & (best < BIG), best & 255, lab)
    return out.astype(np.uint8)


def tables(seed=0):
    """The four tables of the kernel tests: every track, a random subset, none, and all with entry 0 set (which is ignored)."""
    rng = np.random.default_rng(seed)
    every = np.ones(256, dtype=np.uint8)
    every[0] = 0
    some = (rng.integers(0, 2, size=256) * rng.integers(1, 256, size=256)).astype(np.uint8)      # (any non-zero value says "grows")
    some[[1, 7]] = 1
    some[[0, 200, 255]] = 0
    return {"all": every, "subset": some, "none": np.zeros(256, dtype=np.uint8), "all+0": np.full(256, 1, dtype=np.uint8)}
