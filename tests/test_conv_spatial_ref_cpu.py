"""The proof that tests/test_conv_spatial_gpu.py can fail and need not: on the cases of tests/_conv_spatial_ref.py (no GPU), every
bound admits an independent float32 evaluation of the documented formula (torch on the CPU; for Winograd the emulation of the
kernels' own order of operations) and rejects the seeded mistakes, each applied to the float64 reference on listed cases; the case
lists reach every loop count, tile raggedness and guard of the launchers, restated in the helper's geometry functions."""
import pytest
import torch
import torch.nn.functional as F

import _conv_spatial_ref as R

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, v in sorted(WORST.items()):
        print(f"\ntest_conv_spatial_ref_cpu: {group}: worst float32-CPU err / bound {v:.3f}")


def admit(group, out, ref, bound, what):
    ratio, _, _ = R.worst_ratio(out, ref, bound)
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    R.check_within(out, ref, bound, what)
    assert ratio < 1.0, (what, ratio)


def rejected_somewhere(what, trials):
    """`trials`: (case name, mutant, ref, bound) of every listed case the mistake applies to; at least one must reject it."""
    hits = []
    for name, mutant, ref, bound in trials:
        assert mutant.shape == ref.shape, (what, name)
        if not R.within(mutant, ref, bound):
            hits.append(name)
    assert hits, f"{what}: the bounds admit this mistake on every listed case"
    print(f"\nrejected: {what} (on {len(hits)} of {len(trials)} cases)")


def sane(ref, bound, what):
    """Nothing is left out: the bound is finite and non-negative at EVERY element and the reference lies within it."""
    assert ref.shape == bound.shape and bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), what
    assert R.within(ref, ref, bound), what


WINO_SMALL = [g for g in R.WINO_CASES if g not in (R.WINO_BIG, R.WINO_BIG_OUT)]     # the cases the seeded mistakes are tried on


# ---- the bounds admit float32 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", R.WINO_CASES, ids=str)
def test_winograd_bound_admits_the_float32_pipeline(geom):
    c = R.wino_case(geom)
    admit("winograd", R.wino_eval(c["x"], c["w"], c["b"], geom[5]), c["ref"], c["bound"], f"winograd {geom}")
    if geom in WINO_SMALL:
        y64 = R.wino_eval(c["x"], c["w"], c["b"], geom[5], torch.float64)        # the pipeline IS the convolution
        assert float((y64 - c["ref"]).abs().max()) < 1e-12


def test_winograd_weight_is_rounded_once():
    for Cout, Cin in R.WINO_WEIGHTS:
        w = torch.randn(Cout, 3, 3, Cin, generator=R._gen(Cout, Cin))
        u64 = R.wino_weight64(w)
        G = R.rows_matrix(((((0, 1),), ((0, .5), (1, .5), (2, .5)), ((0, .5), (1, -.5), (2, .5)), ((2, 1),))), 3)
        if Cin <= 96:
            assert float((torch.einsum("ar,nrsc,bs->abnc", G, w.double(), G).reshape(16, Cout, Cin) - u64).abs().max()) < 1e-14
        admit("winograd weight", R.wino_weight(w), u64, R.U * u64.abs(), f"winograd weight {Cout} x {Cin}")


@pytest.mark.parametrize("geom", R.STEM_CASES, ids=str)
def test_stem_bound_admits_float32(geom):
    c = R.stem_case(geom)
    admit("stem_conv", R.stem_ref(c["frames"], geom[3], geom[4], c["w"], c["b"], torch.float32), c["ref"], c["bound"], f"stem {geom}")


@pytest.mark.parametrize("geom", R.IM2COL_CASES, ids=str)
def test_stem_im2col_bound_admits_float32(geom):
    f = R.stem_frames(geom[0], geom[1], geom[2], geom[5])
    ref = R.im2col_ref(f, geom[3], geom[4])
    assert bool((ref[:, 147:] == 0).all()) and ref.shape == (R.im2col_geometry(geom)["rows"], 160)
    admit("stem_im2col", R.im2col_ref(f, geom[3], geom[4], torch.float32), ref, 2 * R.U * ref.abs(), f"stem_im2col {geom}")


def test_stem_reference_is_the_im2col_product():
    """The two references agree: im2col rows times the [64, 147] weight matrix, bias, ReLU, in float64."""
    geom = R.STEM_CASES[2]
    c = R.stem_case(geom)
    col = R.im2col_ref(c["frames"], geom[3], geom[4])[:, :147]
    y = torch.relu(col @ c["w"].double().reshape(64, 147).t() + c["b"].double())
    assert float((y.view(c["ref"].shape) - c["ref"]).abs().max()) < 1e-12


@pytest.mark.parametrize("geom", R.DW_CASES, ids=str)
def test_depthwise_bound_admits_float32(geom):
    kernel, NI, H, W, C, up2 = geom
    c = R.dw_case(geom)
    x = c["x"].permute(0, 3, 1, 2)
    if up2:                                                        # independently: torch's own ConvTranspose2d and grouped conv
        x = F.conv_transpose2d(x, c["tw"].view(C, 1, 1, 1), c["tb"], stride=2, output_padding=1, groups=C)
    out = F.conv2d(x, c["wt"].t().reshape(C, 1, 5, 5), c["bias"], padding=2, groups=C).permute(0, 2, 3, 1)
    admit(f"depthwise {kernel}", out, c["ref"], c["bound"], f"depthwise {geom}")
    if kernel == "quad":                                           # and the quad kernel's own formula, in float32
        z = torch.zeros(C)
        ones = torch.ones_like(R.up2_virtual(c["x"], c["tw"], z))
        out = c["bias"] + c["tb"] * R.dw_taps(ones, c["wt"]) + c["tw"] * R.dw_taps(R.up2_virtual(c["x"], torch.ones(C), z), c["wt"])
        admit("depthwise quad", out, c["ref"], c["bound"], f"depthwise {geom} as bias + tb sum(w) + tw sum(w x)")


@pytest.mark.parametrize("geom", R.POOL_CASES, ids=str)
def test_maxpool_reference_is_torch_max_pool(geom):
    c = R.pool_case(geom)
    assert torch.equal(c["ref"], F.max_pool2d(c["x"].permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))


@pytest.mark.parametrize("geom", R.UP_CASES, ids=str)
def test_upsample_index_rule_is_interpolate_nearest(geom):
    NI, H, W, Hb, Wb, C = geom
    c = R.up_case(geom)
    want = c["a"] + F.interpolate(c["b"].permute(0, 3, 1, 2), size=(H, W), mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(c["ref"], want)
    pos = torch.arange(Hb * Wb, dtype=torch.float32).view(1, 1, Hb, Wb)                  # (and index by index)
    idx = F.interpolate(pos, size=(H, W), mode="nearest").long()[0, 0]
    assert torch.equal(idx, R.up_index(H, Hb)[:, None] * Wb + R.up_index(W, Wb)[None, :])


# ---- the case lists reach every branch ----------------------------------------------------------------------------------------------
def test_case_lists_reach_every_branch():
    Rg = R
    wg = {g: Rg.wino_geometry(g) for g in Rg.WINO_CASES}
    T = {v["T"] for v in wg.values()}
    assert min(T) < 32 and any(t > 128 and t % 64 and t % 128 for t in T) and 64 in T             # fewer rows than a tile, ragged, exact
    assert {g[4] for g in Rg.WINO_CASES} >= {4, 36, 64, 100, 260} and {g[3] for g in Rg.WINO_CASES} >= {32, 96, 160}
    assert {g[5] for g in Rg.WINO_CASES} == set(Rg.WINO_ACTS) and {g[6] for g in Rg.WINO_CASES} == {True, False}
    assert {g[7] for g in Rg.WINO_CASES} >= {0, 4, 64} and any(g[8] > 0 for g in Rg.WINO_CASES)
    small = [g for g in Rg.WINO_CASES if g[1] <= 8 and g[2] <= 8]
    assert {g[1] for g in small} | {g[2] for g in small} >= {1, 2, 3, 5, 8} and {g[0] for g in small} == {1, 3}
    assert any(g[1] % 2 and g[2] % 2 for g in small) and any(g[1] % 2 == 0 and g[2] % 2 == 0 for g in small)   # both sides of the odd-edge guard
    big = wg[Rg.WINO_BIG]
    assert big["per_img"] > Rg.GROUP_BYTES and big["group"] == 1 and big["loops_in"] == {1, 2}
    # (a third trip of a transform's loop takes over 8192 * 256 * 2 work items: an input, or an output, of over 67 M floats -- not in a quick test)
    out = wg[Rg.WINO_BIG_OUT]
    assert out["per_img"] > Rg.GROUP_BYTES and out["loops_out"] == {1, 2} and out["loops_in"] == {1} and big["loops_out"] == {1}
    assert all(v["loops_in"] == {1} and v["loops_out"] == {1} for g, v in wg.items() if g not in (Rg.WINO_BIG, Rg.WINO_BIG_OUT))
    assert Rg.grid_loops(260 * 4064, 256, 4096) == {1, 2} and (260, 4064) in Rg.WINO_WEIGHTS
    assert set(Rg.WINO_TILES) == {1, 2, 3, 4, 5, 7, 8, 9} and Rg.WINO_RAGGED in Rg.WINO_CASES

    sg = [Rg.stem_geometry(g) for g in Rg.STEM_CASES]
    loops = set().union(*(v["loops"] for v in sg))
    assert loops >= {1, 2, 3} and any(v["ntiles"] == 1 for v in sg) and any(v["ntiles"] > 768 for v in sg)
    assert {v["ragged"] for v in sg} >= {(True, True), (False, False)}
    assert any(g[5] for g in Rg.STEM_CASES) and any(not g[5] for g in Rg.STEM_CASES) and any(g[6] > 0 for g in Rg.STEM_CASES)
    assert any(g[1] == 1 and g[2] == 1 for g in Rg.STEM_CASES) and any(g[1] == 1 for g in Rg.STEM_CASES) and any(g[2] == 1 for g in Rg.STEM_CASES)
    ig = [Rg.im2col_geometry(g) for g in Rg.IM2COL_CASES]
    assert set().union(*(v["loops"] for v in ig)) >= {1, 2, 3} and any(v["rows"] > 26215 for v in ig) and any(v["rows"] < 100 for v in ig)

    for kernel in ("c256", "quad", "generic"):
        cases = [g for g in Rg.DW_CASES if g[0] == kernel]
        geo = [Rg.dw_geometry(g) for g in cases]
        assert set().union(*(v["loops"] for v in geo)) >= {1, 2, 3}, kernel
        assert {(g[2], g[3]) for g in cases} >= set(Rg.DW_SMALL), kernel
        assert any(v["interior"] for v in geo) and any(not v["interior"] for v in geo), kernel
    assert any(v["odd_w"] for v in map(Rg.dw_geometry, Rg.DW_CASES) if "odd_w" in v) and any(not Rg.dw_geometry(g)["odd_w"] for g in Rg.DW_CASES if g[0] == "c256")
    assert any(Rg.dw_geometry(g)["both_borders"] for g in Rg.DW_CASES if g[0] == "quad")
    assert {g[4] for g in Rg.DW_CASES if g[0] == "generic"} >= {4, 32, 252} and {g[5] for g in Rg.DW_CASES if g[0] == "generic"} == {True, False}

    pg = [Rg.pool_geometry(g) for g in Rg.POOL_CASES]
    assert set().union(*(v["loops"] for v in pg)) >= {1, 2, 3}
    assert {g[1] for g in Rg.POOL_CASES} | {g[2] for g in Rg.POOL_CASES} >= {1, 2, 3, 4, 31, 48} and {g[3] for g in Rg.POOL_CASES} == {4, 64}
    assert any(g[4] for g in Rg.POOL_CASES)
    ug = [Rg.up_geometry(g) for g in Rg.UP_CASES]
    assert set().union(*(v["loops"] for v in ug)) >= {1, 2, 3}
    pairs = {(g[1], g[3]) for g in Rg.UP_CASES} | {(g[2], g[4]) for g in Rg.UP_CASES}
    assert pairs >= {(6, 3), (45, 23), (23, 12), (15, 7), (20, 9), (1, 1), (5, 5)}


def test_nothing_is_left_out():
    """Every element of every case has a finite bound that the reference itself meets: the share left out is zero."""
    for g in R.WINO_CASES:
        c = R.wino_case(g)
        assert c["ref"].shape == (g[0], g[1], g[2], g[4])
        sane(c["ref"], c["bound"], f"winograd {g}")
    for g in R.STEM_CASES:
        c = R.stem_case(g)
        assert c["ref"].shape == (g[0], g[3] // 2, g[4] // 2, 64)
        sane(c["ref"], c["bound"], f"stem {g}")
    for g in R.DW_CASES:
        c = R.dw_case(g)
        k = 2 if g[5] else 1
        assert c["ref"].shape == (g[1], k * g[2], k * g[3], g[4])
        sane(c["ref"], c["bound"], f"depthwise {g}")


# ---- the bounds reject the seeded mistakes ----------------------------------------------------------------------------------------
def test_winograd_mistakes_are_rejected():
    mistakes = {f"sign flipped in row {r} of B^T": dict(bt=R.flip_sign(R.BT_ROWS, r, 1)) for r in range(4)}
    mistakes.update({f"sign flipped in row {r} of A^T": dict(at=R.flip_sign(R.AT_ROWS, r, 1)) for r in range(2)})
    mistakes["transform indices a / b swapped"] = dict(swap_ab=True)
    mistakes["tiles addressed (tx, ty) for (ty, tx)"] = dict(swap_tiles=True)
    mistakes["padding replicated instead of zero"] = dict(pad="replicate")
    mistakes["bias added before the output transform"] = dict(bias_first=True)
    for what, kw in mistakes.items():
        rejected_somewhere(f"winograd: {what}", [(str(g), R.wino_eval(R.wino_case(g)["x"], R.wino_case(g)["w"], R.wino_case(g)["b"], g[5],
                                                                      torch.float64, **kw), R.wino_case(g)["ref"], R.wino_case(g)["bound"]) for g in WINO_SMALL])
    rejected_somewhere("winograd: activation dropped", [(str(g), R.wino_eval(R.wino_case(g)["x"], R.wino_case(g)["w"], R.wino_case(g)["b"], None,
                                                                              torch.float64), R.wino_case(g)["ref"], R.wino_case(g)["bound"])
                                                        for g in WINO_SMALL if g[5] is not None])
    trials, tails = [], []
    for g in WINO_SMALL:
        if g[1] % 2 == 0 and g[2] % 2 == 0:
            continue
        c = R.wino_case(g)
        full = R.wino_eval(c["x"], c["w"], c["b"], g[5], torch.float64, crop=False)
        body, tail = R.wino_store_unguarded(full, g[1], g[2], 2 * g[2] + 2)
        trials.append((str(g), body, c["ref"], c["bound"]))
        tails.append(bool(torch.isfinite(tail).any()))
    rejected_somewhere("winograd: the odd-edge guard removed (a store to row H or column W)", trials)
    assert any(tails)                                                                    # ... and it reaches the band behind the output


def test_stem_mistakes_are_rejected():
    mistakes = {"pad 2 for 3": dict(pad=2), "the canvas beyond the image normalised as (0 - mean) / sd": dict(canvas_raw_zero=True),
                "channels swapped": dict(channels=(2, 1, 0)), "a tile computed from the previous tile's patch": dict(prev_tile=True)}
    for what, kw in mistakes.items():
        rejected_somewhere(f"stem: {what}", [(str(g), R.stem_ref(R.stem_case(g)["frames"], g[3], g[4], R.stem_case(g)["w"], R.stem_case(g)["b"], **kw),
                                              R.stem_case(g)["ref"], R.stem_case(g)["bound"]) for g in R.STEM_CASES[2:]])
    big = R.STEM_CASES[0]                                                               # the persistent loop's case tells the stale patch too
    c = R.stem_case(big)
    assert not R.within(R.stem_ref(c["frames"], big[3], big[4], c["w"], c["b"], prev_tile=True), c["ref"], c["bound"])


def test_depthwise_mistakes_are_rejected():
    small = [g for g in R.DW_CASES if g[2] * g[3] < 1000]
    def trials(sel, **kw):
        return [(str(g), R.dw_ref(R.dw_case(g)["x"], R.dw_case(g)["wt"], R.dw_case(g)["bias"], g[5], R.dw_case(g)["tw"], R.dw_case(g)["tb"], **kw),
                 R.dw_case(g)["ref"], R.dw_case(g)["bound"]) for g in small if sel(g)]
    for kernel in ("c256", "quad", "generic"):
        rejected_somewhere(f"depthwise {kernel}: kh / kw transposed", trials(lambda g: g[0] == kernel, transpose=True))
    for kernel in ("quad", "generic"):
        rejected_somewhere(f"depthwise {kernel}: up2 parity wrong", trials(lambda g: g[0] == kernel and g[5], parity=1))
        rejected_somewhere(f"depthwise {kernel}: tb counted at out-of-image taps", trials(lambda g: g[0] == kernel and g[5], tb_outside=True))
    rejected_somewhere("depthwise quad: a border quad given the interior constant", trials(lambda g: g[0] == "quad", interior_bottom_right=True))


def test_exact_kernels_tell_their_mistakes():
    hits = [g for g in R.POOL_CASES[:-1] if not torch.equal(R.maxpool_ref(R.pool_case(g)["x"], init=0.0), R.pool_case(g)["ref"])]
    assert all(g in hits for g in R.POOL_CASES[:-1] if g[4])                            # every all-negative input shows it
    print(f"\nrejected: max pool: initial value 0 (on {len(hits)} cases)")
    hits = [g for g in R.POOL_CASES[:-1] if not torch.equal(R.maxpool_ref(R.pool_case(g)["x"], shift=1), R.pool_case(g)["ref"])]
    assert hits
    print(f"\nrejected: max pool: window shifted by one (on {len(hits)} cases)")
    hits = [g for g in R.UP_CASES[:-1] if not torch.equal(R.upsample_add_ref(R.up_case(g)["a"], R.up_case(g)["b"], torch.round), R.up_case(g)["ref"])]
    assert hits
    print(f"\nrejected: upsample: round for floor (on {len(hits)} cases)")
