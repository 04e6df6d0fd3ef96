"""The host-side pieces of mdqe_cvpr2023_amd/merge.py that every output path shares, without a GPU: the RLE-dict builder
(rle.positions_to_rles / rle.empty_rle) against rle.encode_dense and against a decode of its own strings, and the stitcher
(merge.stitch, merge.stitch_rles, merge.track_geometry) against a direct construction: a table of the whole video filled with
"empty" and overwritten window by window.  Everything compared is integers, bools and strings: exact."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mdqe_cvpr2023_amd import merge, rle as R  # noqa: E402

H, W = 13, 9
WINDOWS = ((0, 4, 0), (4, 4, 2), (8, 3, 2), (11, 4, 5), (15, 2, 6))       # (f_off, frames, tracks): none at first, then growing
L = 17


def _masks(n, nf, seed):
    """Random blobs; mask (0, 0) all zero, mask (n-1, nf-1) all one, mask (0, nf-1) a single pixel in the last position."""
    rng = np.random.default_rng(seed)
    m = rng.random((n, nf, H, W)) < rng.random((n, nf, 1, 1))
    if n:
        m[0, 0] = False
        m[n - 1, nf - 1] = True
        if n > 1:
            m[0, nf - 1] = False
            m[0, nf - 1, H - 1, W - 1] = True
    return m


def _positions(m, slack):
    """What ops.final_masks_rle returns for these masks: per mask the column-major pixel indices at which the value changes (0 before
    the first pixel), in a buffer `slack` columns wider than the longest list, the unused tail filled with garbage."""
    flat = m.reshape(-1, H, W)
    lists = [np.flatnonzero(np.diff(np.concatenate([[0], f.flatten(order="F").astype(np.int8)])) != 0) for f in flat]
    cap = max([len(p) for p in lists] + [1]) + slack
    pos = np.full((len(lists), cap), -7, dtype=np.int32)
    for i, p in enumerate(lists):
        pos[i, :len(p)] = p
    return pos, np.array([len(p) for p in lists], dtype=np.int32)


def _decode(d):
    counts, lengths = R.strings_to_counts([d["counts"]])
    assert int(counts.sum()) == d["size"][0] * d["size"][1]
    v = np.repeat(np.arange(len(counts)) % 2 == 1, counts)
    return v.reshape(d["size"][1], d["size"][0]).T


def _window_pieces():
    return [(f, nf, n, _masks(n, nf, seed=10 + k)) for k, (f, nf, n) in enumerate(WINDOWS)]


def test_rle_dicts_equal_the_dense_encoder_and_decode_to_the_masks():
    for slack in (0, 5):
        for f_off, nf, n, m in _window_pieces():
            if not n:
                continue
            pos, n_pos = _positions(m, slack)
            got = R.positions_to_rles(pos, n_pos, (H, W), nf)
            assert len(got) == n and all(len(g) == nf for g in got)
            for i in range(n):
                for f in range(nf):
                    assert got[i][f] == R.encode_dense(m[i, f]), (f_off, i, f)
                    assert np.array_equal(_decode(got[i][f]), m[i, f]), (f_off, i, f)
    zero = np.zeros((H, W), dtype=bool)
    assert R.empty_rle((H, W)) == R.encode_dense(zero) and not _decode(R.empty_rle((H, W))).any()
    one = R.positions_to_rles(np.zeros((1, 1), dtype=np.int32), np.array([1], dtype=np.int32), (H, W), 1)[0][0]
    assert one == R.encode_dense(~zero) and _decode(one).all()


ROWS = [3, 0, 5, 1, 3, 4]                                   # outputs: any order, one track twice, tracks that appear late


def test_stitch_dense_masks():
    wins = [(f, nf, n, torch.from_numpy(m)) for f, nf, n, m in _window_pieces()]
    want = torch.zeros(6, L, H, W, dtype=torch.bool)
    for f, nf, n, m in wins:
        want[:n, f:f + nf] = m
    for windows in (wins, [w for w in wins if w[2]]):       # the offline early path does not record windows without tracks
        got = merge.stitch(ROWS, L, windows, lambda k: torch.zeros((k, H, W), dtype=torch.bool), torch.cat)
        assert len(got) == len(ROWS)
        for j, r in enumerate(ROWS):
            assert got[j].dtype == torch.bool and torch.equal(got[j], want[r]), (j, r)
    first = {r: next(f for f, nf, n, m in wins if r < n) for r in ROWS}
    assert first[5] == 15 and not bool(want[5, :15].any()) and bool(want[5, 15:].any())


def test_stitch_rle_lists():
    pieces = _window_pieces()
    wins = [(f, nf, n, [[R.encode_dense(m[i, k]) for k in range(nf)] for i in range(n)]) for f, nf, n, m in pieces]
    dense = np.zeros((6, L, H, W), dtype=bool)
    for f, nf, n, m in pieces:
        dense[:n, f:f + nf] = m
    for windows in (wins, [w for w in wins if w[2]]):
        got = merge.stitch_rles(ROWS, L, (H, W), windows)
        for j, r in enumerate(ROWS):
            assert got[j] == [R.encode_dense(dense[r, k]) for k in range(L)], (j, r)


def test_track_geometry_is_the_stitched_table():
    pieces = _window_pieces()
    wins = [(f, nf, n, R.geometry_dense(torch.from_numpy(m))) for f, nf, n, m in pieces]
    dense = torch.zeros(6, L, H, W, dtype=torch.bool)
    for f, nf, n, m in pieces:
        dense[:n, f:f + nf] = torch.from_numpy(m)
    boxes, areas = R.geom_to_boxes(R.geometry_dense(dense))
    for windows in (wins, [w for w in wins if w[2]], [(f, nf, n, g.numpy()) for f, nf, n, g in wins]):
        got = merge.track_geometry(ROWS, L, (H, W), windows)
        assert sorted(got) == ["pred_areas", "pred_boxes"]
        for j, r in enumerate(ROWS):
            assert got["pred_boxes"][j].dtype == torch.float32 and torch.equal(got["pred_boxes"][j], boxes[r]), (j, r)
            assert got["pred_areas"][j].dtype == torch.int64 and torch.equal(got["pred_areas"][j], areas[r]), (j, r)
    a, b = got["pred_areas"][0], got["pred_areas"][4]       # ROWS[0] == ROWS[4]: two outputs of one track do not share storage
    a[0] = -5
    assert int(b[0]) != -5
