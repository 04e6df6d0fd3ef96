"""The occlusion table without a GPU: the two forms of its reference and the three identities of the rule, the helpers of occlusion.py,
the stitching of the windows' tables, the forms, the property, the refusals and the ABI."""
import dataclasses
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _matte_ref as MREF  # noqa: E402
import _occlusion_ref as REF  # noqa: E402


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def _case(k, Fw, seed, integer):
    Hm, Wm, h, w, Ho, Wo = 5, 7, 18, 26, 13, 21
    rng = np.random.default_rng(seed)
    lg = rng.integers(-3, 4, size=(k, Fw, Hm, Wm)).astype(np.float32) if integer else rng.standard_normal((k, Fw, Hm, Wm)).astype(np.float32)
    return MREF.oracle_values(torch.from_numpy(lg), h, w, Ho, Wo)


@pytest.mark.parametrize("k,integer", [(1, True), (4, True), (6, False), (0, True)])
def test_the_two_forms_of_the_reference_agree_and_the_three_identities_hold(k, integer):
    v, bits = _case(k, 2, seed=10 + k, integer=integer)
    occ, tied = REF.table(v, bits)
    assert occ.dtype == np.int32 and occ.shape == (k, 2, k)
    assert np.array_equal(occ, REF.table_pixelwise(v, bits))
    if k == 4:
        assert tied >= 1 and int((occ * (1 - np.eye(k, dtype=np.int32))[:, None, :]).sum()) >= 1     # ties and overlaps really occur
    o, _ = REF.owner(v, bits)
    for r in range(k):
        assert np.array_equal(occ[r, :, r], (o == r).reshape(2, -1).sum(1))           # 1: the diagonal is the visible region's area
        assert np.array_equal(occ[r].sum(-1), bits[r].reshape(2, -1).sum(1))          # 2: the row's sum is the dense mask's area
        for j in range(k):                                                            # 3: off the diagonal, the part of r that j hides
            assert np.array_equal(occ[r, :, j], (bits[r] & (o == j)).reshape(2, -1).sum(1))
    assert np.array_equal((o >= 0), bits.any(0)) if k else bool((o == -1).all())


def test_a_row_listed_twice_is_owned_by_its_earlier_position():
    v, bits = _case(3, 1, seed=3, integer=True)
    v2, b2 = v[[2, 0, 2]], bits[[2, 0, 2]]
    occ, _ = REF.table(v2, b2)
    assert int(occ[:, :, 2].sum()) == 0 and np.array_equal(occ[0], occ[2]) and int(occ[2, :, 0].sum()) > 0
    assert np.array_equal(occ, REF.table_pixelwise(v2, b2))


def test_from_planes_is_the_same_count():
    v, bits = _case(4, 2, seed=14, integer=True)
    occ, _ = REF.table(v, bits)
    o, _ = REF.owner(v, bits)
    ids = [7, 2, 9, 4]
    labels = np.where(o >= 0, np.asarray(ids)[np.maximum(o, 0)] + 1, 0).astype(np.uint8)
    assert np.array_equal(REF.from_planes(bits, labels, ids), occ)


# ---- the helpers -----------------------------------------------------------------------------------------------------------------------
def test_helpers_on_hand_made_tables():
    from mdqe_cvpr2023_amd import occlusion as H
    #               frame 0                    frame 1
    occ = np.array([[[10, 3, 3], [0, 0, 0]],                          # track 0: hidden by 1 and 2 alike (a tie); empty in frame 1
                    [[0, 5, 0], [2, 4, 6]],                           # track 1: whole in frame 0; mostly behind 2 in frame 1
                    [[1, 0, 7], [0, 0, 9]]], dtype=np.int32)
    for kind in (np.asarray, torch.from_numpy):
        t = kind(occ)
        back = (lambda r: r.numpy()) if torch.is_tensor(t) else (lambda r: r)
        assert type(H.area(t)) is type(t)
        assert back(H.area(t)).tolist() == [[16, 0], [5, 12], [8, 9]] and back(H.area(t)).dtype == np.int64
        assert back(H.visible(t)).tolist() == [[10, 0], [5, 4], [7, 9]]
        hf = back(H.hidden_fraction(t))
        assert hf.dtype == np.float64 and hf.tolist() == [[6 / 16, 0.0], [0.0, 8 / 12], [1 / 8, 0.0]]
        idx, cnt = H.top_occluder(t)
        assert back(idx).tolist() == [[1, -1], [-1, 2], [0, -1]] and back(cnt).tolist() == [[3, 0], [0, 6], [1, 0]]
        front = back(H.in_front(t))
        assert front.dtype == bool and front.shape == (3, 2, 3)
        assert front[0, 0].tolist() == [False, True, True] and front[2, 0].tolist() == [False, False, False]
        assert front[1, 1].tolist() == [True, False, True] and not front[:, :, [0, 1, 2]][[0, 1, 2], :, [0, 1, 2]].any()
    # a video's table: the extra column counts as an occluder (index n) and has no row in `in_front`
    vid = np.concatenate([occ, np.array([[[0], [0]], [[9], [6]], [[0], [0]]], dtype=np.int32)], -1)
    assert H.area(vid).tolist() == [[16, 0], [14, 18], [8, 9]] and H.visible(vid).tolist() == [[10, 0], [5, 4], [7, 9]]
    idx, cnt = H.top_occluder(vid)
    assert idx.tolist() == [[1, -1], [3, 2], [0, -1]] and cnt.tolist() == [[3, 0], [9, 6], [1, 0]]      # (6 == 6 in frame 1: the smaller index)
    assert H.in_front(vid).shape == (3, 2, 3) and np.array_equal(H.in_front(vid), H.in_front(occ))
    assert H.hidden_fraction(vid)[1].tolist() == [9 / 14, 14 / 18]
    # no tracks, and what is not a table
    e = np.zeros((0, 4, 0), dtype=np.int32)
    assert H.area(e).shape == (0, 4) and H.top_occluder(e)[0].shape == (0, 4) and H.in_front(e).shape == (0, 4, 0)
    one = np.array([[[5]]], dtype=np.int32)
    assert H.top_occluder(one)[0].tolist() == [[-1]] and H.hidden_fraction(one).tolist() == [[0.0]]
    for bad in (np.zeros((2, 3, 4), dtype=np.int32), np.zeros((2, 2), dtype=np.int32), np.zeros((2, 3, 2))):
        with pytest.raises(ValueError, match="a table is integer"):
            H.area(bad)


# ---- stitching -------------------------------------------------------------------------------------------------------------------------
def test_stitching_hand_made_window_tables():
    from mdqe_cvpr2023_amd import merge
    rng = np.random.default_rng(5)
    w0 = torch.from_numpy(rng.integers(0, 50, size=(2, 3, 2)).astype(np.int32))        # frames 0..2: rows 0, 1
    w1 = torch.from_numpy(rng.integers(0, 50, size=(4, 2, 4)).astype(np.int32))        # frames 3..4: rows 0..3 (2 and 3 appear here)
    wins = [(0, 3, 2, w0), (3, 2, 4, w1)]
    rows = [3, 0, 2]                                                                   # row 1 is not in the output: the last column
    out = merge.occlusion_result(rows, 5, wins)["pred_occlusion"]
    assert out.dtype == torch.int32 and tuple(out.shape) == (3, 5, 4)
    assert not out[0, :3].any() and not out[2, :3].any()                               # before the track's first window: zero
    assert torch.equal(out[1, :3, 1], w0[0, :, 0]) and not out[1, :3, [0, 2]].any()    # row 0 in window 0: rows 3 and 2 do not exist yet
    assert torch.equal(out[1, :3, 3], w0[0, :, 1])                                     # ... and what row 1 hides lands in the last column
    for a, r in enumerate(rows):
        for b, c in enumerate(rows):
            assert torch.equal(out[a, 3:, b], w1[r, :, c])
        assert torch.equal(out[a, 3:, 3], w1[r, :, 1])
    # the row sums are kept: nothing is lost between the columns
    assert torch.equal(out[1].sum(-1), torch.cat([w0[0].sum(-1), w1[0].sum(-1)]))
    # a track behind two outputs: its column is repeated, the last column counts it once as inside
    dup = merge.occlusion_result([0, 0], 5, wins)["pred_occlusion"]
    assert torch.equal(dup[0], dup[1]) and torch.equal(dup[0, :, 0], dup[0, :, 1])
    assert torch.equal(dup[0, 3:, 2], w1[0].sum(-1).int() - w1[0, :, 0])
    # numpy tables are taken too; a video with no tracks; a window without tracks
    assert torch.equal(merge.occlusion_result(rows, 5, [(f, nf, n, t.numpy()) for f, nf, n, t in wins])["pred_occlusion"], out)
    none = merge.occlusion_result([], 5, [(0, 5, 0, torch.zeros(0, 5, 0, dtype=torch.int32))])["pred_occlusion"]
    assert none.dtype == torch.int32 and tuple(none.shape) == (0, 5, 1)
    late = merge.occlusion_result([0], 5, [(0, 3, 0, torch.zeros(0, 3, 0, dtype=torch.int32)), (3, 2, 1, torch.tensor([[[4], [6]]], dtype=torch.int32))])
    assert late["pred_occlusion"].tolist() == [[[0, 0], [0, 0], [0, 0], [4, 0], [6, 0]]]


# ---- forms, property, refusals -----------------------------------------------------------------------------------------------------------
def test_forms_carry_the_flag_and_matte_is_still_the_last_field():
    from mdqe_cvpr2023_amd.merge import EarlyMasks, Forms
    names = [f.name for f in dataclasses.fields(Forms)]
    assert names[-1] == "matte" and names[-2] == "occlusion" and Forms().occlusion is False

    class Old:
        pass
    assert Forms.of_model(Old()) == Forms(planes="dense")                             # a stand-in without the attribute: the old Forms

    class New:
        occlusion_output = True
    assert Forms.of_model(New()) == Forms(planes="dense", occlusion=True) and Forms.of_model(New(), emit_masks=False) == Forms()
    for emit in ("masks", "rle", "labels", "overlay"):
        f = Forms.of_emit(emit, occlusion=True)
        assert f.occlusion and f == dataclasses.replace(Forms.of_emit(emit), occlusion=True) and not Forms.of_emit(emit).occlusion
    assert not Forms.of_emit("rle", occlusion=True).labels                            # the table needs no label map
    assert Forms.of_emit("overlay", surface=True, occlusion=True).surface
    assert EarlyMasks(done=None).occlusion == []


def _standin(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)
    ns = types.SimpleNamespace(cfg=cfg, device=torch.device("cuda", 0))
    ns.check_label_capacity = lambda: MDQE.check_label_capacity(ns)
    ns.check_occlusion_capacity = lambda: MDQE.check_occlusion_capacity(ns)
    return ns


def test_online_session_takes_the_option_beside_every_emit_and_the_window_fields_are_unchanged():
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.online import Window
    for emit in ("masks", "rle", "labels", "overlay"):
        assert MDQE.online_video(_standin(), emit=emit, occlusion=True).occlusion is True
    assert MDQE.online_video(_standin(), emit="overlay", surface=True, occlusion=True).occlusion is True
    assert MDQE.online_video(_standin(), emit="masks").occlusion is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="occlusion must be a bool"):
            MDQE.online_video(_standin(), emit="masks", occlusion=bad)
    with pytest.raises(ValueError, match="COCO image config.*video config"):
        MDQE.online_video(_standin(is_coco=True), emit="masks", occlusion=True)
    with pytest.raises(ValueError, match="n_max_inst.*exceeds.*255.*lower it"):
        MDQE.online_video(_standin(n_max_inst=256), emit="rle", occlusion=True)
    assert [f.name for f in dataclasses.fields(Window)] == ["frames", "track_ids", "cls_probs", "masks", "rles", "boxes", "areas"]
    w = Window(frames=(0, 2), track_ids=[0], cls_probs=torch.zeros(1, 2), occlusion="o")
    assert w.occlusion == "o" and w.matte is None and Window(frames=(0, 2), track_ids=[], cls_probs=None).occlusion is None


def test_model_property_validation_and_the_three_refusals():
    from mdqe_cvpr2023_amd import sharding
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.merge import Forms
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    m = MDQE(PRESETS["R50_ovis_360"], seed=1)
    assert m.occlusion_output is False and Forms.of_model(m) == Forms(planes="dense")
    m.occlusion_output = True
    assert m.occlusion_output is True and Forms.of_model(m) == Forms(planes="dense", occlusion=True)
    m.label_output = "only"
    assert Forms.of_model(m) == Forms(labels=True, occlusion=True)
    m.label_output = False
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="occlusion_output must be False or True"):
            m.occlusion_output = bad
    assert m.occlusion_output is True
    m.occlusion_output = False
    assert Forms.of_model(m) == Forms(planes="dense")
    with pytest.raises(ValueError, match="n_max_inst.*exceeds.*255.*lower it"):       # more than 255 rows
        MDQE(dataclasses.replace(PRESETS["R50_ovis_360"], n_max_inst=256), seed=1).occlusion_output = True
    coco = types.SimpleNamespace(cfg=dataclasses.replace(m.cfg, is_coco=True), engine=None, device=torch.device("cpu"), occlusion_output=True)
    with pytest.raises(ValueError, match="COCO image branch has no occlusion table.*video config"):
        MDQE.inference_image(coco, [{"image": torch.zeros(3, 3, 8, 8)}])
    geo = types.SimpleNamespace(Hp=8, Wp=8, N=4)
    model = types.SimpleNamespace(cfg=m.cfg, device=torch.device("cpu"), engine=types.SimpleNamespace(geometry=lambda h, w: geo), occlusion_output=True)
    with pytest.raises(ValueError, match="occlusion_output is not offered by the sharded driver.*one device"):
        sharding.run_round_robin(model, {0: torch.zeros(4, 3, 8, 8)}, [(0, 0, 4)], 0, 1, None, (8, 8))


# ---- the ABI and the wrapper ---------------------------------------------------------------------------------------------------------------
def test_header_table_and_exported_symbol_agree_and_bad_arguments_are_refused():
    from mdqe_cvpr2023_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    name = "mdqe_final_masks_occlusion"
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    assert hasattr(h, name) and len(proto.split(",")) == len(_lib.SIGNATURES[name]) == 13
    plan = re.search(r"\bint\s+%s_plan\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    assert hasattr(h, name + "_plan") and len(plan.split(",")) == len(_lib.SIGNATURES[name + "_plan"]) == 5
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # a new entry only
    EINVAL, ENULL = 1, 3

    def occ(n_sel=2, Fw=1, Hm=4, Wm=6, factor=4, h_=16, w=24, Ho=16, Wo=24):
        return h.mdqe_final_masks_occlusion(None, n_sel, None, Fw, Hm, Wm, factor, h_, w, Ho, Wo, None, None)
    for kw in ({"n_sel": 256}, {"n_sel": -1}, {"Fw": -1}, {"Ho": 0}, {"h_": 17}, {"factor": 0}, {"Ho": 1 << 16, "Wo": 1 << 15},
               {"Hm": 1 << 16, "Wm": 1 << 15, "h_": 16}, {"n_sel": 255, "Fw": 40000}):
        assert occ(**kw) == EINVAL, kw                                                            # ... before any pointer is looked at
    assert occ(Fw=0) == 0 and occ(n_sel=0) == 0 and occ(n_sel=0, Fw=0) == 0                       # nothing to do: OK, nothing launched
    assert occ(n_sel=256, Fw=0) == EINVAL
    assert occ() == ENULL


def test_the_launch_plan_keeps_every_count_inside_the_blocks_table_for_every_n_sel():
    """The library's own plan, from the kernel's own row-to-table-row mapping: for every n_sel the chunks tile the k axis, a block packs
    bits of ITS chunk's rows only (a bit of another chunk's row would be counted past the block's table, where the hardware drops the
    access and no result shows it), the table index of every (row, owner) pair lies inside the LDS the launch asks for, and that fits
    the 64 KB a block gets."""
    import ctypes
    from mdqe_cvpr2023_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    chunk, chunks, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    slots = (ctypes.c_int * (8 * 255))()
    args = [ctypes.addressof(x) for x in (chunk, chunks, lds)]
    for bad in (0, -1, 256):
        assert h.mdqe_final_masks_occlusion_plan(bad, *args, None) == 1
    assert h.mdqe_final_masks_occlusion_plan(5, None, args[1], args[2], None) == 3
    seen = {}
    for n in range(1, 256):
        for j in range(len(slots)):
            slots[j] = -7
        assert h.mdqe_final_masks_occlusion_plan(n, *args, ctypes.addressof(slots)) == 0
        c, nc, nbytes = chunk.value, chunks.value, lds.value
        seen[n] = nc
        assert 1 <= c <= 128 and 1 <= nc <= 8 and (nc - 1) * c < n <= nc * c, n          # two 64-bit words a lane; no empty chunk
        assert nbytes == 4 * (n + c * n) and nbytes <= 64 * 1024, n                     # ids[n] | tab[c, n]
        for b in range(nc):
            k0, kc = b * c, min(c, n - b * c)
            row = [slots[b * n + k] for k in range(n)]
            assert row == [k - k0 if k0 <= k < k0 + kc else -1 for k in range(n)], (n, b)
            assert 4 * (n + max(row) * n + (n - 1)) < nbytes                            # the farthest count a block can aim at
        assert all(s == -7 for s in slots[nc * n:nc * n + 4])                           # nothing written past the plan
    assert [n for n in range(2, 256) if seen[n] != seen[n - 1]] == [128, 181, 220, 253] and seen[255] == 5 and seen[127] == 1


def test_the_wrapper_checks_shapes_and_dtypes_before_devices():
    from mdqe_cvpr2023_amd import ops
    lg, idx = torch.zeros(2, 1, 4, 6), torch.arange(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="logits must be"):
        ops.final_occlusion(torch.zeros(2, 4, 6), idx, 4, 16, 24, 16, 24)
    with pytest.raises(RuntimeError, match="inst_idx must be int32"):
        ops.final_occlusion(lg, idx.long(), 4, 16, 24, 16, 24)
    with pytest.raises(RuntimeError, match="inst_idx must be int32"):
        ops.final_occlusion(lg, torch.zeros(256, dtype=torch.int32), 4, 16, 24, 16, 24)
    for bad in (torch.zeros(2, 1, 2), torch.zeros(2, 2, 2, dtype=torch.int32), torch.zeros(2, 1, 4, dtype=torch.int32)[..., ::2]):
        with pytest.raises(RuntimeError, match="out must be contiguous int32"):
            ops.final_occlusion(lg, idx, 4, 16, 24, 16, 24, bad)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.final_occlusion(lg, idx, 4, 16, 24, 16, 24, torch.zeros(2, 1, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.final_occlusion(lg, idx, 4, 16, 24, 16, 24)
