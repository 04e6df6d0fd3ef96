"""Host helpers on an occlusion table (ops.final_occlusion, `win.occlusion`, "pred_occlusion").

A table `occ` is integer [n, F, n] (a window's: rows and columns are its tracker rows) or [n, F, n + 1] (a video's: rows and the first n
columns are the outputs in the order of "pred_track_ids", the last column the tracks that are not among them): occ[k, f, j] = the pixels
of track k's final mask in frame f that track j owns -- j == k: k's visible region; j != k: the part of k that j hides.  Every helper
takes a numpy array or a host torch tensor, of either layout, and answers in kind.
"""
import numpy as np


def _np(occ):
    """-> (the table as int64 numpy [n, F, n or n + 1], a function that gives a result the caller's kind)."""
    try:
        import torch
        is_t = torch.is_tensor(occ)
    except ImportError:                                   # (numpy alone is enough for numpy tables)
        is_t = False
    a = occ.detach().cpu().numpy() if is_t else np.asarray(occ)
    if a.ndim != 3 or a.shape[2] not in (a.shape[0], a.shape[0] + 1) or a.dtype.kind not in "iu":
        raise ValueError("occlusion: a table is integer [n, F, n] or [n, F, n + 1], got %s %s" % (a.dtype, a.shape))
    if is_t:
        import torch
        return a.astype(np.int64), lambda r: torch.from_numpy(np.ascontiguousarray(r))
    return a.astype(np.int64), lambda r: r


def area(occ):
    """int64 [n, F]: the pixels of each track's final mask (the row's sum: every set pixel has exactly one owner)."""
    a, back = _np(occ)
    return back(a.sum(-1))


def visible(occ):
    """int64 [n, F]: the pixels of each track's visible region, the ones it owns itself (the diagonal)."""
    a, back = _np(occ)
    k = np.arange(a.shape[0])
    return back(a[k, :, k])


def hidden_fraction(occ):
    """float64 [n, F]: the share of each track's mask that other tracks own, (area - visible) / area; 0 where the area is 0."""
    a, back = _np(occ)
    k = np.arange(a.shape[0])
    tot, vis = a.sum(-1), a[k, :, k]
    out = np.zeros(tot.shape, dtype=np.float64)
    np.divide(tot - vis, tot, out=out, where=tot > 0)
    return back(out)


def top_occluder(occ):
    """-> (index int64 [n, F], pixels int64 [n, F]): per track and frame the column with the largest off-diagonal count -- the track
    that hides most of it, the smallest index on a tie; in a video's table the index n stands for the tracks that are not among the
    outputs -- and that count; index -1 and 0 pixels where nothing hides the track."""
    a, back = _np(occ)
    off = a.copy()
    k = np.arange(a.shape[0])
    off[k, :, k] = 0
    if off.shape[2] == 0:
        z = np.zeros(off.shape[:2], dtype=np.int64)
        return back(z - 1), back(z)
    idx = off.argmax(-1).astype(np.int64)                  # (numpy: the FIRST maximum)
    cnt = np.take_along_axis(off, idx[..., None], -1)[..., 0]
    return back(np.where(cnt > 0, idx, -1)), back(cnt)


def in_front(occ):
    """bool [n, F, n]: true at (k, f, j) where occ[k, f, j] > occ[j, f, k] (a video's extra column has no row to compare with and is
    left out)."""
    a, back = _np(occ)
    n = a.shape[0]
    sq = a[:, :, :n]
    return back(sq > sq.transpose(2, 1, 0))
