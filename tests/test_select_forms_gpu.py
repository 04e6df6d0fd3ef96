"""Every dispatch branch of the query-selection, clip and post-decoder kernels (decoder_ops.hip: score_max, cell_argmax,
sample_levels_mean; clip_ops.hip: all sixteen kernels; mask.hip: mask_row_stats; image_ops.hip: image_mask_stats, image_final_masks)
against the float64 restatements of tests/_select_ref.py, element by element: a launch passes only if EVERY element lies within
its own derived bound, every decision obeys the margin rule (decided: equal to float64; undecided: one of the contenders), and
nothing outside the documented output was written -- every output is a view of a larger buffer pre-filled with a sentinel bit
pattern (the scheme of tests/test_gemm_forms_gpu.py), and where the header says that only part of a buffer is written (kept past
n_keep, the tiles of sim that hold no pair, rows of sel / out past n_sel) the rest must still hold the sentinel.  The entry points
are called through the C ABI with workspaces of this test's own, so every intermediate (order, n_thr, inv_norm, sim, soft_h, hard_h,
stats, mi) is checked.  tests/test_select_ref_cpu.py shows on the same cases that the checks admit the formulas in float32 and
reject twenty-one one-off mistakes.  The achieved err / bound of every kernel group goes to the parity-margin table."""
import ctypes

import pytest
import torch

import _select_ref as R
from _golden import record_margin
from test_gemm_forms_gpu import SENT

pytestmark = pytest.mark.gpu

COUNT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\ntest_select_forms_gpu: {sum(COUNT.values())} launches compared element by element")
    for branch, n in sorted(COUNT.items()):
        print(f"    {n:5d}  {branch}")


def launched(*branches):
    for b in branches:
        COUNT[b] = COUNT.get(b, 0) + 1


def margins(group, stage, res):
    for name, (err, b) in res.items():
        record_margin("select " + group, f"{stage} {name}".strip(), err, scale=b if b > 0 else 1.0, tol=1.0)


# ---- canary ---------------------------------------------------------------------------------------------------------------------
FRONT = 256                         # words before a view (1 KiB: every view is 16-byte aligned)


def sent(shape, dtype=torch.float32, tail=4096):
    """(buffer, view): a contiguous view of `shape` and `dtype`, FRONT words into a sentinel-filled int32 buffer with `tail` words behind it."""
    n = 1
    for s in (shape if isinstance(shape, (tuple, list)) else (shape,)):
        n *= s
    words = n if dtype != torch.uint8 else (n + 3) // 4
    buf = torch.full((FRONT + words + tail,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf[FRONT:FRONT + words].view(dtype)[:n].view(shape)


def check_sent(buf, view, what, written=None):
    """The sentinel must stand outside the view and on the view's elements outside `written` (a bool mask of the view's shape; None:
    all of it is written), and must be gone from every written element."""
    n = view.numel()
    if view.dtype == torch.uint8:
        hit, start = buf.view(torch.uint8) == torch.full_like(buf, SENT).view(torch.uint8), FRONT * 4
    else:
        hit, start = buf == SENT, FRONT
    w = torch.ones(n, dtype=torch.bool, device="cuda") if written is None else written.reshape(-1).cuda()
    inside = hit[start:start + n]
    ok = torch.stack([hit[:start].all() & hit[start + n:].all(), inside[~w].all(), ~inside[w].any()]).tolist()
    assert ok[0], f"{what}: wrote outside the buffer's view"
    assert ok[1], f"{what}: wrote where the header says nothing is written"
    assert ok[2], f"{what}: left documented elements unwritten"


def ints(v):
    return (ctypes.c_int * max(len(v), 1))(*[int(x) for x in v])


def api():
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    return check, cur_stream, lib, ptr


# ---- query_select ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.QS_SHAPES)
def test_query_select_score_map_cells_and_coordinates(shape):
    check, cur_stream, lib, ptr = api()
    NI, H, W, K, nb = shape
    for vs in R.QS_SETS + R.QS_EXACT:
        c = R.qs_case(*shape, vs)
        what = f"query_select {shape} {vs}"
        conf = c["conf"].cuda()
        sb, score = sent((NI, H, W))
        cb, coords = sent((NI, nb * nb, 2))
        check(lib.mdqe_query_select_f32(ptr(conf), NI, H, W, K, nb, ptr(score), ptr(coords), cur_stream()), what)
        check_sent(sb, score, what + " score")
        check_sent(cb, coords, what + " coords")
        margins("query_select", vs, R.qs_verify(c, score.cpu(), coords.cpu()))
        launched("score_max", R.qs_branch(H, W, nb))
    check(lib.mdqe_query_select_f32(ptr(conf), 0, H, W, K, nb, ptr(score), ptr(coords), cur_stream()), "NI = 0")       # writes nothing
    sb2, s2 = sent((4,))
    check(lib.mdqe_query_select_f32(ptr(conf), 0, H, W, K, nb, ptr(s2), ptr(s2), cur_stream()), "NI = 0")
    check_sent(sb2, s2, "query_select NI = 0", written=torch.zeros(4, dtype=torch.bool))
    launched("query_select NI = 0")


# ---- sample_levels_mean ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,C,front", R.SLM_CASES)
def test_sample_levels_mean(levels, C, front):
    check, cur_stream, lib, ptr = api()
    for vs in R.SLM_SETS:
        c = R.slm_case(levels, C, front, vs)
        what = f"sample_levels_mean {levels} C={C} front={front} {vs}"
        tok, coords = c["tok"].cuda(), c["coords"].cuda()
        NI, N, _ = tok.shape
        Qn, n = coords.shape[1], len(c["shapes"])
        ob, out = sent((NI, Qn, C))
        hs, ws, st = ints([s[0] for s in c["shapes"]]), ints([s[1] for s in c["shapes"]]), ints(c["starts"])
        check(lib.mdqe_sample_levels_mean_f32(ptr(tok), NI, N, C, ptr(coords), Qn, hs, ws, st, n, ptr(out), cur_stream()), what)
        check_sent(ob, out, what)
        res = {}
        R.need_within(res, "out", out.cpu(), c["ref"], c["bound"], what)
        margins("sample_levels_mean", vs, res)
        launched(f"sample_levels_mean {n} level{'s' if n > 1 else ''}")


# ---- clip_assoc, clip_gather_init -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ASSOC_CASES)
def test_clip_assoc_and_gather_init(case):
    check, cur_stream, lib, ptr = api()
    E, Q, T, wdw, Bc = case
    for vs in R.ASSOC_SETS:
        c = R.assoc_case(*case, vs)
        what = f"clip_assoc {case} {vs}"
        emb, fidx = c["emb"].cuda(), c["fidx"].cuda()
        ib, idx = sent((Bc, T, Q), torch.int32)
        check(lib.mdqe_clip_assoc_f32(ptr(emb), Q, E, ptr(fidx), Bc, T, c["ct"], float(wdw), c["nb"], ptr(idx), cur_stream()), what)
        check_sent(ib, idx, what)
        margins("clip_assoc", vs, R.assoc_verify(c, idx.cpu()))
        launched(f"clip_assoc<{E}> {(Q + 63) // 64} block{'s' if Q > 64 else ''}")
        content, coords = c["content"].cuda(), c["coords"].cuda()
        C = content.shape[-1]
        for use_idx in ((True, False) if vs == "normal" else (True,)):
            xb, x = sent((Bc, T, Q, C))
            rb, ref = sent((Bc, T, Q, 4))
            nb_, xi = sent((Bc, Q, C))
            check(lib.mdqe_clip_gather_init_f32(ptr(content), ptr(coords), ptr(fidx), ptr(idx) if use_idx else None, Bc, T, Q, C, c["ct"], ptr(x),
                                                ptr(ref), ptr(xi), cur_stream()), what)
            for b_, v_ in ((xb, x), (rb, ref), (nb_, xi)):
                check_sent(b_, v_, what + " gather_init")
            ex, er, ei = R.gather_init_ref(c["content"], c["coords"], c["fidx"], idx.cpu() if use_idx else None, c["ct"])
            assert torch.equal(x.cpu(), ex) and torch.equal(ref.cpu(), er) and torch.equal(xi.cpu(), ei), what + " gather_init"
            margins("clip_gather_init", "exact", {"x, ref, x_inst": (0.0, 1.0)})
            launched("clip_gather_init" + ("" if use_idx else " idx = NULL"))
    check(lib.mdqe_clip_assoc_f32(ptr(emb), Q, E, ptr(fidx), 0, T, c["ct"], float(wdw), c["nb"], ptr(idx), cur_stream()), "Bc = 0")


# ---- box_refine, box_head_refine ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.BOX_CASES)
def test_box_refine(case):
    check, cur_stream, lib, ptr = api()
    Bc, T, Q, which = case
    for vs in R.BOX_SETS:
        c = R.box_case(*case, vs)
        what = f"box_refine {case} {vs}"
        delta, prev = c["delta"].cuda(), c["prev"].cuda()
        bb, boxes = sent((Bc, T, Q, 4))
        ib, ibox = sent((Bc, Q, 4))
        check(lib.mdqe_box_refine_f32(ptr(delta), ptr(prev), Bc, T, Q, c["t0"], c["t1"], ptr(boxes), ptr(ibox), cur_stream()), what)
        check_sent(bb, boxes, what + " boxes")
        check_sent(ib, ibox, what + " ibox")
        margins("box_refine", vs, R.box_verify(c, boxes.cpu(), ibox.cpu(), what))
        launched("box_refine")


@pytest.mark.parametrize("case", R.HEAD_CASES)
def test_box_head_refine_against_float64_and_bit_equal_to_the_two_kernel_form(case):
    check, cur_stream, lib, ptr = api()
    from mdqe_cvpr2023_amd import ops
    Bc, T, Q, K, ldh, which = case
    c = R.head_case(*case)
    what = f"box_head_refine {case}"
    hbuf = torch.randn(Bc * T * Q, ldh, device="cuda")
    hbuf[:, :K] = c["h"].cuda()
    h, W, bias, prev = hbuf[:, :K], c["W"].cuda(), c["bias"].cuda(), c["prev"].cuda()
    bb, boxes = sent((Bc, T, Q, 4))
    ib, ibox = sent((Bc, Q, 4))
    check(lib.mdqe_box_head_refine_f32(ptr(h), ldh, ptr(W), ptr(bias), ptr(prev), Bc, T, Q, K, c["t0"], c["t1"], ptr(boxes), ptr(ibox),
                                       cur_stream()), what)
    check_sent(bb, boxes, what + " boxes")
    check_sent(ib, ibox, what + " ibox")
    margins("box_head_refine", f"K={K}", R.box_verify(c, boxes.cpu(), ibox.cpu(), what))
    launched(f"box_head_refine K={K}")
    delta = ops.linear(h.contiguous(), W, bias)                                   # the two-kernel form: N = 4 takes the row-dot kernel
    b2, i2 = ops.box_refine(delta, prev.view(-1, 4), Bc, T, Q, c["t0"], c["t1"])
    margins("box_refine", "after linear", R.box_verify(c, b2.cpu(), i2.cpu(), what + " (two kernels)"))
    assert torch.equal(b2.view(-1), boxes.view(-1)) and torch.equal(i2.view(-1), ibox.view(-1)), what + ": fused and two-kernel forms differ"


# ---- time_fuse, time_fuse_dot ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FUSE_CASES)
def test_time_fuse(case):
    check, cur_stream, lib, ptr = api()
    Bc, T, Q, C = case
    for vs in R.FUSE_SETS:
        c = R.fuse_case(*case, vs)
        w, x, pos = c["w"].cuda(), c["x"].cuda(), c["pos"].cuda()
        for with_pos in (False, True):
            what = f"time_fuse {case} {vs} pos={with_pos}"
            ob, out = sent((Bc, Q, C))
            pb, out2 = sent((Bc, Q, C))
            check(lib.mdqe_time_fuse_f32(ptr(w), ptr(x), Bc, T, Q, C, ptr(out), ptr(pos) if with_pos else None, ptr(out2) if with_pos else None,
                                         cur_stream()), what)
            check_sent(ob, out, what)
            check_sent(pb, out2, what + " out + pos", written=None if with_pos else torch.zeros(Bc, Q, C, dtype=torch.bool))
            res = {}
            R.need_within(res, "out", out.cpu(), c["ref"][0], c["bound"][0], what)
            if with_pos:
                R.need_within(res, "out + pos", out2.cpu(), c["ref"][1], c["bound"][1], what)
            margins("time_fuse", vs, res)
            launched("time_fuse" + (" + pos" if with_pos else ""))


@pytest.mark.parametrize("case", R.FUSE_DOT_CASES)
def test_time_fuse_dot_against_float64_and_bit_equal_to_the_two_kernel_form(case):
    check, cur_stream, lib, ptr = api()
    from mdqe_cvpr2023_amd import ops
    Bc, T, Q = case
    for vs in R.FUSE_SETS:
        c = R.fuse_dot_case(*case, vs)
        what = f"time_fuse_dot {case} {vs}"
        xw, wt, bt, src = c["xw"].cuda(), c["wt"].cuda(), c["bt"].cuda(), c["src"].cuda()
        ob, out = sent((Bc, Q, 256))
        check(lib.mdqe_time_fuse_dot_f32(ptr(xw), ptr(wt), ptr(bt), ptr(src), Bc, T, Q, 256, ptr(out), cur_stream()), what)
        check_sent(ob, out, what)
        res = {}
        R.need_within(res, "out", out.cpu(), c["ref"], c["bound"], what)
        margins("time_fuse_dot", vs, res)
        launched("time_fuse_dot")
        w = ops.linear(xw.view(-1, 256), wt.view(1, 256), bt)                          # N = 1: the row-dot kernel
        two = ops.time_fuse(w.view(-1), src.view(-1, 256), Bc, T, Q)
        assert torch.equal(two.view(-1), out.view(-1)), what + ": fused and two-kernel forms differ"


# ---- add_rows, rows_gather ------------------------------------------------------------------------------------------------------
def test_add_rows_and_rows_gather_are_exact():
    check, cur_stream, lib, ptr = api()
    g = torch.Generator().manual_seed(5)
    for rows, C, lda, ldb, ldo in ((1, 4, 4, 4, 4), (37, 64, 72, 64, 68), (300, 256, 256, 260, 264), (5, 8, 16, 12, 8)):
        a, b = torch.randn(rows, lda, generator=g).cuda(), torch.randn(rows, ldb, generator=g).cuda()
        ob, out = sent((rows, ldo))
        check(lib.mdqe_add_rows_f32(ptr(a), lda, ptr(b), ldb, ptr(out), ldo, rows, C, cur_stream()), "add_rows")
        written = torch.zeros(rows, ldo, dtype=torch.bool)
        written[:, :C] = True
        check_sent(ob, out, f"add_rows {rows}x{C}", written)
        assert torch.equal(out[:, :C], a[:, :C] + b[:, :C])
        margins("add_rows", "exact", {"out": (0.0, 1.0)})
        launched("add_rows" + (" pitched" if (lda, ldb, ldo) != (C, C, C) else ""))
    check(lib.mdqe_add_rows_f32(ptr(a), lda, ptr(b), ldb, ptr(out), ldo, 0, C, cur_stream()), "add_rows rows = 0")
    for n_src, length, idx in ((5, 4, [4, 0, 0, 3, 4, 4, 1]), (3, 1028, [2, 2, 0]), (2, 40000, [1, 0, 1])):     # 40 000 floats: more than 32 blocks cover
        src = torch.randn(n_src, length, generator=g).cuda()
        ix = torch.tensor(idx, dtype=torch.int32).cuda()
        ob, out = sent((len(idx), length))
        check(lib.mdqe_rows_gather_f32(ptr(src), ptr(ix), len(idx), length, ptr(out), cur_stream()), "rows_gather")
        check_sent(ob, out, f"rows_gather len {length}")
        assert torch.equal(out, src[ix.long()])
        margins("rows_gather", "exact", {"out": (0.0, 1.0)})
        launched("rows_gather")
    ob, out = sent((4,))
    check(lib.mdqe_rows_gather_f32(ptr(src), ptr(ix), 0, length, ptr(out), cur_stream()), "rows_gather n = 0")
    check_sent(ob, out, "rows_gather n = 0", torch.zeros(4, dtype=torch.bool))


# ---- clip_select ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SELECT_CASES)
def test_clip_select_every_intermediate(case):
    check, cur_stream, lib, ptr = api()
    Q, K, C, n_want, max_keep = case
    for vs in R.SELECT_SETS:
        c = R.select_case(*case, vs)
        what = f"clip_select {case} {vs}"
        B = len(n_want)
        cls, emb = c["cls"].cuda(), c["emb"].cuda()
        (ob, order), (tb, n_thr), (vb, inv), (sb, sim) = sent((B, Q), torch.int32), sent((B,), torch.int32), sent((B, Q)), sent((B, Q, Q))
        (kb, kept), (nb_, n_keep) = sent((B, Q), torch.int32), sent((B,), torch.int32)
        check(lib.mdqe_clip_select_f32(ptr(cls), ptr(emb), B, Q, K, C, float(c["thr"]), max_keep, ptr(order), ptr(n_thr), ptr(inv), ptr(sim),
                                       ptr(kept), ptr(n_keep), cur_stream()), what)
        nk = n_keep.cpu()
        for b_, v_, name, w in ((ob, order, "order", None), (tb, n_thr, "n_thr", None), (vb, inv, "inv_norm", None), (nb_, n_keep, "n_keep", None),
                                (sb, sim, "sim", torch.stack([r["computed"] for r in c["ref"]])),
                                (kb, kept, "kept", torch.arange(Q)[None] < nk[:, None])):
            check_sent(b_, v_, f"{what} {name}", w)
        margins("clip_select", vs, R.select_verify(c, order.cpu(), n_thr.cpu(), inv.cpu(), sim.cpu(), kept.cpu(), nk))
        for r in c["ref"]:
            launched("clip_rank", "clip_dedup", f"clip_gram {'one tile' if r['n_thr'] <= 64 else 'several tiles'}")
    (kb, kept), (nb_, n_keep) = sent((4,), torch.int32), sent((4,), torch.int32)
    check(lib.mdqe_clip_select_f32(ptr(cls), ptr(emb), 0, Q, K, C, float(c["thr"]), max_keep, ptr(order), ptr(n_thr), ptr(inv), ptr(sim),
                                   ptr(kept), ptr(n_keep), cur_stream()), "B = 0")
    check_sent(kb, kept, "clip_select B = 0", torch.zeros(4, dtype=torch.bool))
    check_sent(nb_, n_keep, "clip_select B = 0", torch.zeros(4, dtype=torch.bool))


# ---- dyn_mask_nms, mask_row_stats -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DYN_CASES)
def test_dyn_mask_nms_every_output(case):
    check, cur_stream, lib, ptr = api()
    M, T, H, W, Q, counts = case
    B, rows = len(counts), sum(counts)
    Ph = -(-T // R.t_step_of(T)) * (H // 2) * (W // 2)
    for vs in R.DYN_SETS:
        c = R.dyn_case(*case, vs)
        what = f"dyn_mask_nms {case[:5]} B={B} {vs}"
        coef, kept, feats = c["coef"].cuda(), c["kept"].cuda(), c["feats"].cuda()
        (lb, logits), (sb, soft), (hb, hard) = sent((rows, T, H, W)), sent((rows, Ph)), sent((rows, Ph))
        (tb, stats), (mb, mi) = sent((rows, 5)), sent((rows,))
        part = torch.empty(lib.mdqe_dyn_mask_workspace_floats(rows, T, H, W) + 64, device="cuda")
        gram = torch.empty(lib.mdqe_nms_workspace_floats(max(counts)) + 64, device="cuda")
        check(lib.mdqe_dyn_mask_nms_f32(ptr(coef), ptr(kept), ptr(feats), B, Q, M, T, H, W, ints(c["row0"]), ints(counts), ints(c["f0"]), ptr(logits),
                                        ptr(soft), ptr(hard), ptr(part), ptr(gram), ptr(stats), ptr(mi), cur_stream()), what)
        for b_, v_, name in ((lb, logits, "logits"), (sb, soft, "soft_h"), (hb, hard, "hard_h"), (tb, stats, "stats"), (mb, mi, "mi")):
            check_sent(b_, v_, f"{what} {name}")
        lg, so, ha, st, m = logits.cpu(), soft.cpu(), hard.cpu(), stats.cpu(), mi.cpu()
        for b, n in enumerate(counts):
            s = slice(c["row0"][b], c["row0"][b] + n)
            margins("dyn_mask_nms", vs, R.dyn_verify(c, b, lg[s], so[s], ha[s], st[s], m[s]))
        launched(*R.dyn_branch(M, T, H, W, counts), "mask_stats_reduce", "mask_iou")


@pytest.mark.parametrize("case", R.ROW_CASES)
def test_mask_row_stats(case):
    check, cur_stream, lib, ptr = api()
    T, H, W, n = case
    step = R.t_step_of(T)
    Ph = -(-T // step) * (H // 2) * (W // 2)
    for vs in R.DYN_SETS:
        c = R.row_case(*case, vs)
        what = f"mask_row_stats {case} {vs}"
        lg = c["logits"].cuda()
        (tb, stats), (sb, soft), (hb, hard) = sent((n, 5)), sent((n, Ph)), sent((n, Ph))
        check(lib.mdqe_mask_row_stats_f32(ptr(lg), n, T, H, W, step, ptr(stats), ptr(soft), ptr(hard), cur_stream()), what)
        for b_, v_, name in ((tb, stats, "stats"), (sb, soft, "soft_h"), (hb, hard, "hard_h")):
            check_sent(b_, v_, f"{what} {name}")
        res = {}
        R.stats_verify(res, c["bounds"], c["ref"][2], soft.cpu(), hard.cpu(), stats.cpu(), what)
        margins("mask_row_stats", vs, res)
        launched(f"mask_row_stats t_step={step}")


# ---- clip_finalize --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FIN_CASES)
def test_clip_finalize(case):
    check, cur_stream, lib, ptr = api()
    Q, K, C, counts = case
    B, rows = len(counts), sum(counts)
    for kind in R.FIN_KINDS:
        c = R.fin_case(*case, kind)
        what = f"clip_finalize {case} {kind}"
        cls, emb, kept, stats, mi = (c[k].cuda() for k in ("cls", "emb", "kept", "stats", "mi"))
        (sb, sel), (nb_, n_sel), (ob, out) = sent((rows,), torch.int32), sent((B,), torch.int32), sent((rows, 2 + K + C))
        check(lib.mdqe_clip_finalize_f32(ptr(cls), ptr(emb), ptr(kept), ptr(stats), ptr(mi), B, Q, K, C, float(c["thr"]), ints(c["row0"]),
                                         ints(counts), ptr(sel), ptr(n_sel), ptr(out), cur_stream()), what)
        ns = n_sel.cpu()
        row_written = torch.zeros(rows, dtype=torch.bool)
        for b in range(B):
            row_written[c["row0"][b]:c["row0"][b] + int(ns[b])] = True
        check_sent(nb_, n_sel, what + " n_sel")
        check_sent(sb, sel, what + " sel", row_written)
        check_sent(ob, out, what + " out", row_written[:, None].expand(rows, 2 + K + C))
        margins("clip_finalize", kind, R.fin_verify(c, ns, sel.cpu(), out.cpu()))
        launched("clip_finalize")


# ---- image_mask_stats, image_final_masks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.IMG_CASES)
def test_image_mask_stats_and_final_masks(case):
    check, cur_stream, lib, ptr = api()
    Hm, Wm, f, h, w, Ho, Wo = case
    for vs in R.IMG_SETS:
        c = R.img_case(*case, vs)
        what = f"image ops {case} {vs}"
        lg, idx = c["lg"].cuda(), c["idx"].cuda()
        n, k = lg.shape[0], idx.numel()
        tb, stats = sent((n, 6))
        check(lib.mdqe_image_mask_stats_f32(ptr(lg), n, Hm, Wm, f, h, w, ptr(stats), cur_stream()), what)
        check_sent(tb, stats, what + " stats")
        margins("image_mask_stats", vs, R.img_stats_verify(c, stats.cpu()))
        mb, masks = sent((k, Ho, Wo), torch.uint8)
        check(lib.mdqe_image_final_masks_u8(ptr(lg), k, ptr(idx), Hm, Wm, f, h, w, Ho, Wo, ptr(masks), cur_stream()), what)
        check_sent(mb, masks, what + " masks")
        margins("image_final_masks", vs, R.img_final_verify(c, masks.cpu()))
        launched(f"image_mask_stats factor {f}", f"image_final_masks factor {f}")
    tb, stats = sent((6,))
    check(lib.mdqe_image_mask_stats_f32(ptr(lg), 0, Hm, Wm, f, h, w, ptr(stats), cur_stream()), "n = 0")
    check(lib.mdqe_image_final_masks_u8(ptr(lg), 0, ptr(idx), Hm, Wm, f, h, w, Ho, Wo, ptr(stats), cur_stream()), "n = 0")
    check_sent(tb, stats, "image ops n = 0", torch.zeros(6, dtype=torch.bool))
