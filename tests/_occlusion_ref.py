"""The rule of mdqe_final_masks_occlusion (include/mdqe_hip.h) restated on the CPU from up-sampled values and final-mask bits
(_matte_ref.oracle_values gives both): occ[k, f, j] = #{(Y, X) : b_k set and o == j}, o the first row with the largest value among the
set ones.  Two forms, vectorised and written pixel by pixel the way the header says it; test_occlusion_cpu.py holds them against each
other, the GPU tests use the vectorised one."""
import numpy as np


def owner(v, bits):
    """v float [k, Fw, Ho, Wo], bits bool -> (o int64 [Fw, Ho, Wo]: the owner's position, -1 where no bit is set; tied bool [Fw, Ho,
    Wo]: the largest value among the set rows is held by two or more of them)."""
    k = v.shape[0]
    if k == 0:
        z = np.zeros(v.shape[1:], dtype=np.int64)
        return z - 1, z.astype(bool)
    score = np.where(bits, v, -np.inf)
    o = score.argmax(0).astype(np.int64)                               # numpy: the FIRST maximum -- the tie rule
    some = bits.any(0)
    tied = ((score == score.max(0)[None]) & bits).sum(0) >= 2
    return np.where(some, o, -1), tied


def table(v, bits):
    """-> (occ int32 [k, Fw, k], the number of pixels whose owner is tied with another set row)."""
    k, Fw = v.shape[:2]
    o, tied = owner(v, bits)
    occ = np.zeros((k, Fw, k), dtype=np.int32)
    for f in range(Fw):
        of = o[f].ravel()
        for r in range(k):
            sel = of[bits[r, f].ravel()]                               # (a set pixel always has an owner)
            occ[r, f] = np.bincount(sel, minlength=k)[:k]
    return occ, int(tied.sum())


def table_pixelwise(v, bits):
    """`table`'s counts pixel by pixel, the way the header writes the rule."""
    k, Fw, Ho, Wo = v.shape
    occ = np.zeros((k, Fw, k), dtype=np.int32)
    for f in range(Fw):
        for Y in range(Ho):
            for X in range(Wo):
                o = -1
                for r in range(k):                                     # the smallest r among the set rows with the largest value
                    if bits[r, f, Y, X] and (o < 0 or v[r, f, Y, X] > v[o, f, Y, X]):
                        o = r
                for r in range(k):
                    if bits[r, f, Y, X]:
                        occ[r, f, o] += 1
    return occ


def from_planes(dense, labels, ids):
    """The table from outputs of the other kernels: dense bool/uint8 [k, F, H, W] (row k's plane) and labels uint8 [F, H, W] (the label
    map), ids[j] + 1 the label of column j -> int64 [k, F, len(ids)]: #{dense[k, f] set and labels[f] == ids[j] + 1}."""
    dense, labels = np.asarray(dense) != 0, np.asarray(labels)
    k, F = dense.shape[:2]
    out = np.zeros((k, F, len(ids)), dtype=np.int64)
    for f in range(F):
        for r in range(k):
            cnt = np.bincount(labels[f][dense[r, f]].ravel(), minlength=256)
            out[r, f] = [cnt[i + 1] for i in ids]
    return out
