"""The occlusion table on the device (ops.final_occlusion) and the surfaces above it (model.occlusion_output, online_video(occlusion=True)).

One definition: occ[k, f, j] = #{(Y, X) : b_k set and o == j}, b_k the final-mask bit of selected row k and o the label map's owner.

Kernel against the CPU reference on logits that take only the values +-1, +-2, +-3 (test_label_map_gpu._int_logits): with factor 4 every
up-sampled value is an exact multiple of 1/16 in fp32, so values, bits and exact ties are the same on the device and on the CPU and every
count is compared exactly.  Float logits: against the untouched dense and label-map kernels, exactly as well -- all three share the device
expressions.  The k axis goes in chunks of at most 16384 / n_sel - 1 rows a block: one chunk up to 127 rows, two up to 180, three up to
219, four up to 252, five beyond; a case stands on each side of every one of those.

Wall time of this file on one MI355X (pytest's own figure, one model construction included): 2.4 s for its 26 tests.  The model cases
run with the class threshold lowered to 1e-6: 43 tracks per window.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _matte_ref as MREF  # noqa: E402
import _occlusion_ref as REF  # noqa: E402
from test_label_map_gpu import FACTOR, SHAPES, _int_logits  # noqa: E402

SMALL = (8, 12, 32, 48, 32, 48)
GARBAGE = -12345


def _run(lg, rows, shape):
    """ops.final_occlusion into a garbage-filled buffer, twice -> the table on the host (int32 numpy [k, Fw, k])."""
    from mdqe_cvpr2023_amd import ops
    Hm, Wm, h, w, Ho, Wo = shape
    dev = lg.cuda()
    idx = torch.tensor(rows, dtype=torch.int32, device="cuda")
    k, Fw = len(rows), int(lg.shape[1])
    out = torch.full((k, Fw, k), GARBAGE, dtype=torch.int32, device="cuda")
    got = ops.final_occlusion(dev, idx, FACTOR, h, w, Ho, Wo, out)
    assert got is out
    first = out.cpu()
    again = ops.final_occlusion(dev, idx, FACTOR, h, w, Ho, Wo, torch.full_like(out, 77))       # other garbage, a buffer of its own
    fresh = ops.final_occlusion(dev, idx, FACTOR, h, w, Ho, Wo)                                 # ... and one the wrapper allocates
    assert fresh.dtype == torch.int32 and tuple(fresh.shape) == (k, Fw, k) and fresh.is_cuda
    assert torch.equal(again.cpu(), first) and torch.equal(fresh.cpu(), first)                  # identical from run to run
    return first.numpy()


def _int_case(lg, rows, shape):
    Hm, Wm, h, w, Ho, Wo = shape
    v, bits = MREF.oracle_values(lg[rows], h, w, Ho, Wo)
    want, tied = REF.table(v, bits)
    got = _run(lg, rows, shape)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    return want, tied, bits


@pytest.mark.parametrize("shape", SHAPES)
def test_integer_logits_against_the_reference(shape):
    Hm, Wm = shape[:2]
    lg = _int_logits(5, 3, Hm, Wm, seed=Hm + shape[5])
    for rows in ([0, 1, 2, 3, 4], [3, 0, 1, 3]):                   # every row; a strict subset in another order, one row listed twice
        want, tied, bits = _int_case(lg, rows, shape)
        k = len(rows)
        off = want.copy()
        off[np.arange(k), :, np.arange(k)] = 0
        assert tied >= 1 and int(off.sum()) >= 1 and int(want.sum()) > 0          # tied pixels and real overlaps are in the case
        assert np.array_equal(want.sum(-1), bits.reshape(k, 3, -1).sum(-1))
    assert int(want[:, :, 3].sum()) == 0 and np.array_equal(want[0], want[3])     # the later position of row 3 owns nothing


@pytest.mark.parametrize("shape", SHAPES)
def test_float_logits_against_the_untouched_kernels(shape):
    from mdqe_cvpr2023_amd import ops
    Hm, Wm, h, w, Ho, Wo = shape
    n, Fw = 6, 4
    lg = torch.randn(n, Fw, Hm, Wm, generator=torch.Generator().manual_seed(Hm * 7 + Ho)) * 2
    dev = lg.cuda()
    rows = [5, 2, 0, 3, 1, 4]
    idx = torch.tensor(rows, dtype=torch.int32, device="cuda")
    dense, dgeom = ops.final_masks_geom(dev, idx, FACTOR, h, w, Ho, Wo, torch.zeros(n, Fw, Ho, Wo, dtype=torch.uint8, device="cuda"), 0)
    labels, lgeom = ops.final_label_map(dev, idx, FACTOR, h, w, Ho, Wo, torch.empty(Fw, Ho, Wo, dtype=torch.uint8, device="cuda"), 0, geom=True)
    occ = torch.from_numpy(_run(lg, rows, shape)).long()
    d, lab = dense.cpu() != 0, labels.cpu()
    want = torch.stack([torch.stack([(d[k] & (lab == rows[j] + 1)).flatten(1).sum(1) for j in range(n)], -1) for k in range(n)])
    assert torch.equal(occ, want)
    assert torch.equal(occ[torch.arange(n), :, torch.arange(n)], lgeom.view(n, Fw, 5)[..., 0].cpu().long())     # the visible regions' areas
    assert torch.equal(occ.sum(-1), dgeom.view(n, Fw, 5)[..., 0].cpu().long())                                  # the dense masks' areas
    assert int((occ.sum(-1) - occ[torch.arange(n), :, torch.arange(n)]).sum()) > 0                              # (something is hidden)


def _chunks(n):
    """The number of chunks the entry launches for n rows: the library's own plan (mdqe_final_masks_occlusion_plan), not a restatement."""
    import ctypes
    from mdqe_cvpr2023_amd import _lib
    chunk, chunks, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    assert _lib.load_library().mdqe_final_masks_occlusion_plan(n, ctypes.addressof(chunk), ctypes.addressof(chunks), ctypes.addressof(lds), None) == 0
    return chunks.value


def test_the_chunk_boundaries_are_where_the_cases_stand():
    assert [n for n in range(2, 256) if _chunks(n) != _chunks(n - 1)] == [128, 181, 220, 253]
    assert [_chunks(n) for n in (1, 127, 128, 180, 181, 219, 220, 252, 253, 255)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5]


@pytest.mark.parametrize("n_sel,Fw,shape", [(1, 1, (16, 24, 60, 90, 60, 90)), (70, 2, (16, 24, 60, 90, 60, 90)), (255, 1, SMALL)]
                         + [(n, 1, SMALL) for n in (127, 128, 180, 181, 219, 220, 252, 253)])
def test_many_rows_and_both_sides_of_every_chunk_boundary(n_sel, Fw, shape):
    lg = _int_logits(n_sel, Fw, shape[0], shape[1], seed=n_sel)
    rows = torch.randperm(n_sel, generator=torch.Generator().manual_seed(n_sel)).tolist()
    want, tied, _ = _int_case(lg, rows, shape)
    if n_sel > 64:
        assert tied >= 1 and int((want.sum((0, 1)) > 0).sum()) > 8              # (many rows really own pixels)
        off = want.sum(1) * (1 - np.eye(n_sel, dtype=np.int64))
        step = -(-n_sel // _chunks(n_sel))
        assert all(int(off[a:a + step].sum()) > 0 for a in range(0, n_sel, step))    # ... and every chunk of the k axis has overlaps


def test_every_pixel_carries_every_bit():
    """All logits positive: every pixel carries n_sel bits and every lane walks n_sel - 1 of them -- the worst case of the counting path."""
    n_sel = 255
    rng = np.random.default_rng(1)
    lg = torch.from_numpy(rng.integers(1, 4, size=(n_sel, 1) + SMALL[:2]).astype(np.float32))
    want, tied, bits = _int_case(lg, list(range(n_sel)), SMALL)
    assert bool(bits.all()) and tied >= 1
    assert np.array_equal(want.sum(-1), np.full((n_sel, 1), 32 * 48)) and np.array_equal(want[0], want[-1])


def test_no_bit_set_and_no_rows():
    from mdqe_cvpr2023_amd import ops
    lg = -torch.ones(5, 2, 16, 24)
    assert not _run(lg, [4, 1, 2], (16, 24, 60, 90, 61, 97)).any()
    got = _run(torch.zeros(0, 2, 16, 24), [], (16, 24, 60, 90, 60, 90))
    assert got.shape == (0, 2, 0)
    got = ops.final_occlusion(torch.zeros(3, 0, 16, 24, device="cuda"), torch.arange(3, dtype=torch.int32, device="cuda"), FACTOR, 60, 90, 60, 90)
    assert tuple(got.shape) == (3, 0, 3)


def test_refused_arguments_come_back_as_errors_without_a_launch():
    from mdqe_cvpr2023_amd import ops
    lg = torch.zeros(2, 1, 4, 6, device="cuda")
    idx = torch.arange(2, dtype=torch.int32, device="cuda")
    out = torch.full((2, 1, 2), GARBAGE, dtype=torch.int32, device="cuda")
    for args in ((4, 17, 24, 16, 24), (4, 16, 25, 16, 24), (0, 16, 24, 16, 24), (4, 16, 24, 0, 24), (4, 16, 24, 1 << 16, 1 << 15)):
        with pytest.raises(RuntimeError, match="final_occlusion.*code 1"):
            ops.final_occlusion(lg, idx, *args, out=out if args[3:] == (16, 24) else None)
    torch.cuda.synchronize()
    assert bool((out == GARBAGE).all())                                          # nothing was launched, nothing cleared


# ---- the layers ------------------------------------------------------------------------------------------------------------------------
from test_overlay_gpu import L, OUT, PLANS, _forward, _model, _online, _same  # noqa: E402


def _with_occlusion(model, frames, **attrs):
    """test_overlay_gpu._forward restores only the attributes it knows: the new one is set and restored here."""
    assert model.occlusion_output is False
    model.occlusion_output = True
    try:
        return _forward(model, frames, **attrs)
    finally:
        model.occlusion_output = False


@pytest.fixture(scope="module")
def video():
    from bench import synth_video
    _, model = _model(n_frames_window_test=6, apply_cls_thres=1e-6)               # (tens of tracks per window)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    plain = _forward(model, frames, label_output=True)
    on = _with_occlusion(model, frames, label_output=True)
    return model, frames, plain, on


def _video_table(res):
    """pred_occlusion recomputed on the host from the run's own pred_masks and pred_label_map."""
    ids = list(res["pred_track_ids"])
    masks = torch.stack(list(res["pred_masks"])).numpy() if ids else np.zeros((0, L) + OUT, dtype=bool)
    lab = res["pred_label_map"].numpy()
    inside = REF.from_planes(masks, lab, ids)
    others = [i for i in range(255) if i not in set(ids)]
    outside = REF.from_planes(masks, lab, others).sum(-1, keepdims=True)
    return torch.from_numpy(np.concatenate([inside, outside], -1).astype(np.int32))


def test_forward_adds_the_table_and_leaves_every_other_output_alone(video):
    model, frames, plain, on = video
    assert set(on) == set(plain) | {"pred_occlusion"} and "pred_occlusion" not in plain
    for k in plain:
        assert _same(on[k], plain[k]), k
    occ, n_out = on["pred_occlusion"], len(on["pred_track_ids"])
    assert occ.dtype == torch.int32 and tuple(occ.shape) == (n_out, L, n_out + 1) and not occ.is_cuda and n_out >= 10
    want = _video_table(on)
    assert torch.equal(occ, want)
    off = occ[:, :, :n_out].clone()
    off[torch.arange(n_out), :, torch.arange(n_out)] = 0
    assert int(off.sum()) > 0 and int(occ[:, :, -1].sum()) > 0                    # tracks hide each other; so do tracks outside the output
    # without the label map, and beside the RLE form: the same table, "pred_track_ids" comes with it
    alone = _with_occlusion(model, frames)
    assert torch.equal(alone["pred_occlusion"], occ) and alone["pred_track_ids"] == on["pred_track_ids"] and "pred_label_map" not in alone
    assert _same(alone["pred_masks"], plain["pred_masks"])
    assert torch.equal(_with_occlusion(model, frames, rle_output=True)["pred_occlusion"], occ)


def test_the_late_mask_path_gives_the_same_table(video):
    model, frames, plain, on = video
    late = _with_occlusion(model, frames, early_masks=False, label_output=True)
    assert set(late) == set(on)
    for k in on:
        assert _same(late[k], on[k]), k


def test_online_windows_carry_their_tables_and_result_equals_forward(video, monkeypatch):
    from mdqe_cvpr2023_amd import ops
    model, frames, plain, on = video
    _, ref_masks, _ = _online(model, frames, [L], emit="masks")
    _, ref_labels, _ = _online(model, frames, [L], emit="labels")
    assert all(w.occlusion is None for w in ref_masks)
    want = [torch.from_numpy(REF.from_planes(m.masks.numpy(), lb.labels.numpy(), list(range(len(m.track_ids)))).astype(np.int32))
            for m, lb in zip(ref_masks, ref_labels)]
    print("tracks per window:", [len(w.track_ids) for w in ref_masks])
    assert max(len(w.track_ids) for w in ref_masks) >= 10
    calls = {"label_map": 0, "occlusion": 0}
    real_map, real_occ = ops.final_label_map, ops.final_occlusion

    def label_map(*a, **kw):
        calls["label_map"] += 1
        return real_map(*a, **kw)

    def occlusion(*a, **kw):
        calls["occlusion"] += 1
        return real_occ(*a, **kw)
    monkeypatch.setattr(ops, "final_label_map", label_map)
    monkeypatch.setattr(ops, "final_occlusion", occlusion)
    for sizes in PLANS:
        calls.update(label_map=0, occlusion=0)
        ov, wins, _ = _online(model, frames, sizes, emit="rle", occlusion=True, keep=True)
        assert [w.frames for w in wins] == [w.frames for w in ref_masks]
        for w, r, t in zip(wins, ref_masks, want):
            n, nf = len(w.track_ids), w.frames[1] - w.frames[0]
            assert w.track_ids == r.track_ids and w.labels is None and w.masks is None and len(w.rles) == n
            assert w.occlusion.dtype == torch.int32 and tuple(w.occlusion.shape) == (n, nf, n) and not w.occlusion.is_cuda
            assert w.occlusion.is_pinned() or n == 0
            assert torch.equal(w.occlusion, t)
        assert calls == {"label_map": 0, "occlusion": len(wins)}                   # the session made no label map
        res = ov.result()
        assert torch.equal(res["pred_occlusion"], on["pred_occlusion"]) and res["pred_track_ids"] == on["pred_track_ids"]
    calls.update(label_map=0, occlusion=0)
    ov, wins, _ = _online(model, frames, [L], emit="rle", keep=True)               # the option off: no sweep, no key
    assert calls == {"label_map": 0, "occlusion": 0} and all(w.occlusion is None for w in wins) and "pred_occlusion" not in ov.result()
    ov, wins, _ = _online(model, frames, [L], emit="overlay", occlusion=True)      # beside a painting session, keep=False: the windows only
    assert all(torch.equal(w.occlusion, t) for w, t in zip(wins, want)) and "pred_occlusion" not in ov.result()
