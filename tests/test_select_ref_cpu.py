"""The proof that tests/test_select_forms_gpu.py can fail and need not: on the cases of tests/_select_ref.py (no GPU), (a) every
check admits an independent float32 evaluation of the formula (torch on the CPU), (b) every check rejects the one-off mistakes of
_select_ref.MISTAKES, each written as a small variant of that float32 evaluation, and (c) the margin rule leaves at most 1 % of
the decisions of any case undecided, computed from the float64 references alone."""
import pytest
import torch

import _select_ref as R

F32 = torch.float32
WORST, REJECTED = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, v in sorted(WORST.items()):
        print(f"\ntest_select_ref_cpu: {group}: worst float32-CPU err / bound {v:.3f}")
    for name, where in sorted(REJECTED.items()):
        print(f"\nrejected: {name} ({R.MISTAKES[name]}) on {where}")


def admit(group, res):
    for name, (err, b) in res.items():
        key = f"{group} {name}"
        WORST[key] = max(WORST.get(key, 0.0), err / b if b > 0 else 0.0)


# ---- one float32 evaluation per group: run(case, mut) -> the verifier's result (raises AssertionError when outside a bound) ------
def run_qs(c, mut=None):
    o = R.qs_eval(c["conf"], c["nb"], F32, mut)
    return R.qs_verify(c, o["score"], o["coords"])


def run_slm(c, mut=None):
    res = {}
    R.need_within(res, "out", R.slm_eval(c["tok"], c["coords"], c["shapes"], c["starts"], F32, mut), c["ref"], c["bound"], "sample_levels_mean")
    return res


def run_assoc(c, mut=None):
    return R.assoc_verify(c, R.assoc_sim(c["emb"], c["fidx"], c["ct"], c["wdw"], c["nb"], F32, mut).argmax(2))


def run_box(c, mut=None):
    return R.box_verify(c, *R.box_eval(c["delta"], c["prev"], c["t0"], c["t1"], F32, mut), "box_refine")


def run_head(c, mut=None):
    d = (c["h"] @ c["W"].t() + c["bias"]).view(c["prev"].shape)
    return R.box_verify(c, *R.box_eval(d, c["prev"], c["t0"], c["t1"], F32, mut), "box_head_refine")


def run_fuse(c, mut=None):
    res = {}
    out, out2 = R.fuse_eval(c["w"], c["x"], c["pos"], F32, mut)
    R.need_within(res, "out", out, c["ref"][0], c["bound"][0], "time_fuse")
    R.need_within(res, "out + pos", out2, c["ref"][1], c["bound"][1], "time_fuse")
    return res


def run_fuse_dot(c, mut=None):
    res = {}
    w = c["xw"] @ c["wt"] + c["bt"]
    R.need_within(res, "out", R.fuse_eval(w, c["src"], torch.zeros_like(c["src"][:, 0]), F32, mut)[0], c["ref"], c["bound"], "time_fuse_dot")
    return res


def run_select(c, mut=None):
    o = R.select_eval(c["cls"], c["emb"], c["thr"], c["max_keep"], F32, mut)
    B, Q = c["cls"].shape[:2]
    kept = torch.full((B, Q), -1, dtype=torch.long)
    for b, r in enumerate(o):
        kept[b, :len(r["kept"])] = r["kept"]
    return R.select_verify(c, torch.stack([r["order"] for r in o]), [r["n_thr"] for r in o], torch.stack([r["inv_norm"] for r in o]),
                           torch.stack([r["sim"] for r in o]), kept, [len(r["kept"]) for r in o])


def run_dyn(c, mut=None):
    res = {}
    for b, o in enumerate(R.dyn_eval(c, F32, mut)):
        for k, v in R.dyn_verify(c, b, *o).items():
            res[k] = max(res.get(k, (0.0, 1.0)), v, key=lambda e: e[0] / e[1] if e[1] > 0 else 0.0)
    return res


def run_row(c, mut=None):
    res = {}
    R.stats_verify(res, c["bounds"], c["ref"][2], *R.stats_eval(c["logits"], F32, mut), "mask_row_stats")
    return res


def run_fin(c, mut=None):
    o = R.fin_eval(c, F32, mut)
    rows = sum(c["counts"])
    sel, out = torch.full((rows,), -1, dtype=torch.long), torch.zeros(rows, 2 + c["K"] + c["C"])
    for b, r in enumerate(o):
        r0 = c["row0"][b]
        sel[r0:r0 + r["n_sel"]] = r["sel"]
        out[r0:r0 + r["n_sel"]] = r["out"]
    return R.fin_verify(c, [r["n_sel"] for r in o], sel, out)


def run_img_stats(c, mut=None):
    return R.img_stats_verify(c, R.img_stats_eval(c["lg"], c["f"], c["h"], c["w"], F32, mut)[1])


def run_img_final(c, mut=None):
    return R.img_final_verify(c, R.img_final_eval(c["lg"], c["idx"], c["f"], c["h"], c["w"], c["Ho"], c["Wo"], F32, mut)[1])


def cases_of(group):
    """[(name, case, run)] of one kernel group: every case and value set of _select_ref."""
    if group == "query_select":
        return [(f"{s} {vs}", R.qs_case(*s, vs), run_qs) for s in R.QS_SHAPES for vs in R.QS_SETS + R.QS_EXACT]
    if group == "sample_levels_mean":
        return [(f"{s} {vs}", R.slm_case(*s, vs), run_slm) for s in R.SLM_CASES for vs in R.SLM_SETS]
    if group == "clip_assoc":
        return [(f"{s} {vs}", R.assoc_case(*s, vs), run_assoc) for s in R.ASSOC_CASES for vs in R.ASSOC_SETS]
    if group == "box_refine":
        return [(f"{s} {vs}", R.box_case(*s, vs), run_box) for s in R.BOX_CASES for vs in R.BOX_SETS] + \
               [(f"head {s}", R.head_case(*s), run_head) for s in R.HEAD_CASES]
    if group == "time_fuse":
        return [(f"{s} {vs}", R.fuse_case(*s, vs), run_fuse) for s in R.FUSE_CASES for vs in R.FUSE_SETS] + \
               [(f"dot {s} {vs}", R.fuse_dot_case(*s, vs), run_fuse_dot) for s in R.FUSE_DOT_CASES for vs in R.FUSE_SETS]
    if group == "clip_select":
        return [(f"{s} {vs}", R.select_case(*s, vs), run_select) for s in R.SELECT_CASES for vs in R.SELECT_SETS]
    if group == "dyn_mask_nms":
        return [(f"{s[:5]} {vs}", R.dyn_case(*s, vs), run_dyn) for s in R.DYN_CASES for vs in R.DYN_SETS] + \
               [(f"row {s} {vs}", R.row_case(*s, vs), run_row) for s in R.ROW_CASES for vs in R.DYN_SETS]
    if group == "clip_finalize":
        return [(f"{s[:3]} {k}", R.fin_case(*s, k), run_fin) for s in R.FIN_CASES for k in R.FIN_KINDS]
    if group == "image_mask_stats":
        return [(f"{s} {vs}", R.img_case(*s, vs), run_img_stats) for s in R.IMG_CASES for vs in R.IMG_SETS]
    if group == "image_final_masks":
        return [(f"{s} {vs}", R.img_case(*s, vs), run_img_final) for s in R.IMG_CASES for vs in R.IMG_SETS]
    raise ValueError(group)


GROUPS = sorted(set(R.MISTAKES.values()))


# ---- (a) the bounds admit float32 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_checks_admit_float32(group):
    for name, case, run in cases_of(group):
        try:
            admit(group, run(case))
        except AssertionError as e:
            raise AssertionError(f"{group} {name}: the check refuses the float32 evaluation: {e}") from None


# ---- (b) the bounds reject the mistakes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake", sorted(R.MISTAKES))
def test_checks_reject_mistake(mistake):
    group = R.MISTAKES[mistake]
    for name, case, run in cases_of(group):
        try:
            run(case, mistake)
        except AssertionError:
            REJECTED[mistake] = name
            return
    raise AssertionError(f"no case of {group} rejects the mistake: {mistake}")


def test_every_kernel_group_has_a_mistake():
    assert set(GROUPS) >= {"query_select", "sample_levels_mean", "clip_assoc", "box_refine", "time_fuse", "clip_select", "dyn_mask_nms",
                           "clip_finalize", "image_mask_stats", "image_final_masks"}


def test_a_mistake_name_the_evaluations_do_not_know_is_not_rejected():
    """The rejection above is the mistake's doing, not the harness's: an unknown name changes nothing and passes."""
    for group in GROUPS:
        name, case, run = cases_of(group)[0]
        run(case, "no such mistake")


# ---- (c) the margin rule leaves little open -------------------------------------------------------------------------------------
def test_undecided_share_is_at_most_one_percent():
    rows = R.undecided_shares()
    worst = max(rows, key=lambda r: r[1] / r[2])
    print(f"\ntest_select_ref_cpu: {len(rows)} cases, {sum(r[1] for r in rows)} of {sum(r[2] for r in rows)} decisions undecided; "
          f"worst {worst[0]}: {worst[1]} of {worst[2]}")
    for name, und, n in rows:
        assert und <= 0.01 * n, (name, und, n)
    for name, und, n in rows:                    # ranks are held to exact equality: none of their decisions may be open
        if name.startswith("clip_finalize"):
            assert und == 0, (name, und)


def test_exact_cases_are_exact_in_float32():
    """The saturated and tied cases: an all-zero score map returns the first pixel of every cell, a single peak the last pixel of cell 0."""
    for shape in R.QS_SHAPES:
        NI, H, W, K, nb = shape
        zero, peak = R.qs_case(*shape, "zero"), R.qs_case(*shape, "peak")
        assert int(zero["ref"]["idx"].abs().max()) == 0
        H_up, W_up, r, t = peak["dims"]
        assert (peak["ref"]["idx"][:, 0] == r * t - 1).all(), shape
        for c in (zero, peak):
            o = R.qs_eval(c["conf"], nb, F32)
            assert torch.equal(o["idx"], c["ref"]["idx"])


def test_image_cases_hold_the_edges_they_are_meant_to():
    """Mask 3 is empty; mask 4's box ends on the crop's bottom-right pixel, and is that pixel alone at the two sizes of the issue that allow it."""
    for s in R.IMG_CASES:
        for vs in R.IMG_SETS:
            c = R.img_case(*s, vs)
            assert tuple(c["stats"][3, 2:].tolist()) == (c["w"], c["h"], -1, -1)
            assert tuple(c["stats"][4, 4:].tolist()) == (c["w"] - 1, c["h"] - 1)
            assert c["pdec"][3:].all()
    assert all(R.img_case(*s, "normal")["corner"] for s in (R.IMG_CASES[0], R.IMG_CASES[2]))
