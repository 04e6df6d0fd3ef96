"""tests/_msda_ref.py checked without a GPU: on the case lists of tests/test_msda_forms_gpu.py every bound admits the formula evaluated
in float32 with plain torch and rejects each seeded one-off mistake on a named case; the input categories are present in the stated
shares; the float64 reference agrees with torch's own grid_sample; and the case lists reach every kernel instantiation the two MSDA
dispatchers can launch, on both sides of every capacity threshold."""
import pytest
import torch
import torch.nn.functional as F

import _msda_ref as R

FUSED_CASES = sorted({n for n, _ in R.FUSED_LAUNCHES})
NATIVE_CASES = sorted(R.NATIVE_SHAPES)
SLM_CASES = sorted(R.SLM_SHAPES)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\ntest_msda_ref_cpu: worst float32 err / bound per group")
    for k in sorted(WORST):
        print(f"    {k}: {WORST[k]:.3f}")


def _family(name):
    return name.split(" ")[0]


def _admit(group, out32, c, what):
    ratio, _, _ = R.worst_ratio(out32, c["out"], c["bound"])
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    R.check_within(out32, c["out"], c["bound"], what)


@pytest.mark.parametrize("name", FUSED_CASES)
def test_fused_bound_admits_the_formula_in_float32(name):
    c = R.fused_case(name)
    _admit("fused " + _family(name), R.fused_eval(c, torch.float32), c, name)
    assert float(c["bound"].max()) < 1e-3 * max(1.0, float(c["out"].abs().max())), "a bound this loose holds nothing"


@pytest.mark.parametrize("name", NATIVE_CASES)
def test_native_bound_admits_the_formula_in_float32(name):
    c = R.native_case(name)
    _admit("native " + _family(name), R.native_eval(c, torch.float32), c, name)


@pytest.mark.parametrize("name", SLM_CASES)
def test_sample_levels_mean_bound_admits_the_formula_in_float32(name):
    c = R.slm_case(name)
    _admit("sample_levels_mean", R.slm_eval(c, torch.float32), c, name)


# mistake -> the case that must reject it
FUSED_MISTAKES = {
    "no_half": "enc 40 D=32",                  # the half-pixel shift dropped
    "swap_xy": "enc 40 D=32",                  # x and y of an offset swapped
    "swap_WH": "enc 40 D=24",                  # W and H swapped in the normalisation
    "no_div8": "v1 L=4 D=16",                  # / 8 dropped
    "clamp_after": "dec Q=65",                 # the clamp applied after the grid term
    "no_clamp": "dec Q=64",                    # the clamp dropped
    "grid_full": "dec 832 builds",             # grid * 0.5 written as grid
    "softmax_P": "enc L2P8 D=32",              # softmax over P instead of L * P
    "level_mod": "enc 40 D=32",                # level taken as i % L instead of i / P
    "start_off1": "enc gap before level 3",    # a level's start row off by one
    "swap_corners": "v1 L=1 D=64",             # corners (h0, w1) and (h1, w0) swapped
    "border": "enc 40 D=32",                   # zero padding replaced by border clamp
    "no_scale": "tp builds",                   # scale dropped
    "drop_group": "v2 two groups",             # one group of G left out
    "no_vidx": "dec B=17",                     # vidx ignored
    "ref_broadcast": "dec Q=1",                # a per-batch ref read as broadcast
}
NATIVE_MISTAKES = {"no_half": "v2 S < 64", "swap_xy": "VEC=2 D=6", "swap_WH": "v3 pyramid", "level_mod": "VEC=4 D=16", "start_off1": "v3 gap and descending",
                   "swap_corners": "VEC=1 D=5", "border": "v2 L2P8", "no_scale": "v2 two groups", "drop_group": "v2 two groups"}
SLM_MISTAKES = {"zero_pad": "four levels", "align_corners": "eight levels C=256", "no_half": "one level C=4", "start_off1": "four levels",
                "swap_corners": "four levels"}


def _border_eval(c, dtype, mistake):
    """`border` is a padding mode of the core, not a mistake flag: zero padding replaced by border clamp."""
    loc, _, _ = R.fused_locations(c, dtype)
    acc = R.sample_sum(R._value3(c, dtype), R._base(c), loc, R.fused_weights(c, dtype), c["levels"], c["G"], c["L"], c["P"], dtype, pad="border")
    return (acc * c["scale"]).reshape(c["B"] * c["Q"], -1)


@pytest.mark.parametrize("mistake", sorted(FUSED_MISTAKES))
def test_fused_bound_rejects(mistake):
    c = R.fused_case(FUSED_MISTAKES[mistake])
    wrong = _border_eval(c, torch.float32, mistake) if mistake == "border" else R.fused_eval(c, torch.float32, mistake)
    assert not R.within(wrong, c["out"], c["bound"]), f"{mistake} passes on {c['name']}"
    assert R.within(R.fused_eval(c, torch.float32), c["out"], c["bound"])


@pytest.mark.parametrize("mistake", sorted(NATIVE_MISTAKES))
def test_native_bound_rejects(mistake):
    c = R.native_case(NATIVE_MISTAKES[mistake])
    if mistake == "border":
        B, S = c["B"], c["S"]
        acc = R.sample_sum(c["value"].view(B * S, c["M"], c["D"]), [b * S for b in range(B)], c["loc"].view(B, c["Q"], c["M"], -1, 2),
                           c["attn"].view(B, c["Q"], c["M"], -1), c["levels"], c["G"], c["L"], c["P"], torch.float32, pad="border")
        wrong = (acc * c["scale"]).reshape(c["out"].shape)
    else:
        wrong = R.native_eval(c, torch.float32, mistake)
    assert not R.within(wrong, c["out"], c["bound"]), f"{mistake} passes on {c['name']}"


@pytest.mark.parametrize("mistake", sorted(SLM_MISTAKES))
def test_sample_levels_mean_bound_rejects(mistake):
    c = R.slm_case(SLM_MISTAKES[mistake])
    assert not R.within(R.slm_eval(c, torch.float32, mistake), c["out"], c["bound"]), f"{mistake} passes on {c['name']}"


def test_every_input_category_is_present():
    """At least 5 % of the look-ups of every case list fall in each category (counted on the float64 locations)."""
    for label, cases, cats in (("fused mode 0", [R.fused_case(n) for n in FUSED_CASES if R.FUSED_SHAPES[n]["mode"] == 0], R.CATEGORIES0),
                               ("fused mode 1", [R.fused_case(n) for n in FUSED_CASES if R.FUSED_SHAPES[n]["mode"] == 1], R.CATEGORIES1),
                               ("native", [R.native_case(n) for n in NATIVE_CASES], R.CATEGORIES0)):
        n = sum(c["cats"]["n"] for c in cases)
        share = {k: sum(c["cats"][k] for c in cases) / n for k in cats}
        print(label, {k: round(v, 3) for k, v in share.items()})
        for k, v in share.items():
            assert v >= R.MIN_SHARE, f"{label}: only {v:.3f} of the look-ups are `{k}`"
    for n in FUSED_CASES:
        s = R.FUSED_SHAPES[n]
        H, W, _ = s["levels"]
        assert all(h != w for h, w in zip(H, W)), n
        c = R.fused_case(n)
        if c["vidx"] is not None and s["B"] >= 3:
            assert c["vidx"] != sorted(c["vidx"]) and c["vidx"] != list(range(s["B"])), n
        if s["mode"] == 1:
            assert bool((c["ref"][..., 2] != c["ref"][..., 3]).all()), n
    assert {R.FUSED_SHAPES[n]["logit_scale"] for n in FUSED_CASES} == {1.0, 30.0}


def test_reference_agrees_with_grid_sample():
    """The float64 sampling core against torch's grid_sample (zeros / border padding, align_corners=False): an independent statement of
    the same interpolation, so the reference does not only agree with itself."""
    c = R.fused_case("enc 40 D=32")
    B, Q, M, D, L, P = (c[k] for k in ("B", "Q", "M", "D", "L", "P"))
    loc, _, _ = R.fused_locations(c, torch.float64)
    w = R.fused_weights(c, torch.float64)
    Hs, Ws, Ss = c["levels"]
    v = c["value"].double().view(B, -1, M, D)
    out = torch.zeros(B, Q, M, D, dtype=torch.float64)
    for l in range(L):
        img = v[:, Ss[l]:Ss[l] + Hs[l] * Ws[l]].permute(0, 2, 3, 1).reshape(B * M, D, Hs[l], Ws[l])
        g = (2 * loc[:, :, :, l * P:(l + 1) * P] - 1).permute(0, 2, 1, 3, 4).reshape(B * M, Q, P, 2)
        s = F.grid_sample(img, g, mode="bilinear", padding_mode="zeros", align_corners=False).view(B, M, D, Q, P)
        out += (s * w[:, :, :, l * P:(l + 1) * P].permute(0, 2, 1, 3)[:, :, None]).sum(-1).permute(0, 3, 1, 2)
    assert float((out.reshape(B * Q, M * D) - c["out"]).abs().max()) < 1e-12
    s = R.slm_case("four levels")
    NI, N, C = s["tokens"].shape
    acc = 0
    for (h, wd), st in zip(s["shapes"], s["starts"]):
        img = s["tokens"].double()[:, st:st + h * wd].view(NI, h, wd, C).permute(0, 3, 1, 2)
        acc = acc + F.grid_sample(img, (2 * s["coords"].double() - 1)[:, :, None], mode="bilinear", padding_mode="border", align_corners=False)[..., 0].transpose(1, 2)
    assert float((acc / len(s["shapes"]) - s["out"]).abs().max()) < 1e-12


def _launches():
    fused = [(n, sw, R.msda_fused_branch(R.FUSED_SHAPES[n], sw)) for n, sw in R.FUSED_LAUNCHES]
    native = [(n, sw, R.msda_native_branch(R.NATIVE_SHAPES[n], sw)) for n, sw in R.NATIVE_LAUNCHES]
    return fused, native


# Every kernel instantiation the two dispatchers can launch, written out from csrc/msda_fused.hip and csrc/msda.hip by hand.
FUSED_BY_HAND = {
    # msda_fused_kernel<L, 4>
    "fused v1 L=1", "fused v1 L=2", "fused v1 L=3", "fused v1 L=4",
    # msda_fused_v2_kernel<4, 4, MAP, WPE, DD>
    "fused v2 L4P4 map=0 waves hint=1 D=32", "fused v2 L4P4 map=0 waves hint=1 D=24", "fused v2 L4P4 map=0 waves hint=8 D=32",
    "fused v2 L4P4 map=0 waves hint=8 D=24", "fused v2 L4P4 map=1 waves hint=1 D=32", "fused v2 L4P4 map=1 waves hint=1 D=24",
    "fused v2 L4P4 map=1 waves hint=8 D=32", "fused v2 L4P4 map=1 waves hint=8 D=24", "fused v2 L4P4 map=2 waves hint=1 D=32",
    "fused v2 L4P4 map=2 waves hint=1 D=24", "fused v2 L4P4 map=2 waves hint=8 D=32", "fused v2 L4P4 map=2 waves hint=8 D=24",
    # msda_fused_v2_kernel<2, 8, MAP, WPE, DD>
    "fused v2 L2P8 map=0 waves hint=1 D=32", "fused v2 L2P8 map=0 waves hint=1 D=24", "fused v2 L2P8 map=0 waves hint=8 D=32",
    "fused v2 L2P8 map=0 waves hint=8 D=24", "fused v2 L2P8 map=1 waves hint=1 D=32", "fused v2 L2P8 map=1 waves hint=1 D=24",
    "fused v2 L2P8 map=1 waves hint=8 D=32", "fused v2 L2P8 map=1 waves hint=8 D=24", "fused v2 L2P8 map=2 waves hint=1 D=32",
    "fused v2 L2P8 map=2 waves hint=1 D=24", "fused v2 L2P8 map=2 waves hint=8 D=32", "fused v2 L2P8 map=2 waves hint=8 D=24",
    # msda_fused_v3_kernel<4, 4, DD, NT>, <.., NT, 0, 2>, <.., NT, 0, 3>
    "fused v3 D=32 threads=512 natural", "fused v3 D=32 threads=512 level 2 at compile time", "fused v3 D=32 threads=512 level 3 at compile time",
    "fused v3 D=32 threads=832 natural", "fused v3 D=32 threads=832 level 2 at compile time", "fused v3 D=32 threads=832 level 3 at compile time",
    "fused v3 D=32 threads=1024 natural", "fused v3 D=32 threads=1024 level 2 at compile time", "fused v3 D=32 threads=1024 level 3 at compile time",
    "fused v3 D=24 threads=512 natural", "fused v3 D=24 threads=512 level 2 at compile time", "fused v3 D=24 threads=512 level 3 at compile time",
    "fused v3 D=24 threads=832 natural", "fused v3 D=24 threads=832 level 2 at compile time", "fused v3 D=24 threads=832 level 3 at compile time",
    "fused v3 D=24 threads=1024 natural", "fused v3 D=24 threads=1024 level 2 at compile time", "fused v3 D=24 threads=1024 level 3 at compile time",
    # msda_fused_v3_kernel<4, 4, DD, 1024, 8> (two blocks per CU) and <4, 4, 32, 832, 8>
    "fused v3 D=32 threads=1024 two blocks", "fused v3 D=24 threads=1024 two blocks", "fused v3 D=32 threads=832 8 waves",
    # msda_fused_tp_kernel<4, 4, 4, DD, NT, -1 | 2 | 3>
    "fused temporal D=32 threads=512 natural", "fused temporal D=32 threads=512 level 2 at compile time", "fused temporal D=32 threads=512 level 3 at compile time",
    "fused temporal D=32 threads=832 natural", "fused temporal D=32 threads=832 level 2 at compile time", "fused temporal D=32 threads=832 level 3 at compile time",
    "fused temporal D=32 threads=1024 natural", "fused temporal D=32 threads=1024 level 2 at compile time", "fused temporal D=32 threads=1024 level 3 at compile time",
    "fused temporal D=24 threads=512 natural", "fused temporal D=24 threads=512 level 2 at compile time", "fused temporal D=24 threads=512 level 3 at compile time",
    "fused temporal D=24 threads=832 natural", "fused temporal D=24 threads=832 level 2 at compile time", "fused temporal D=24 threads=832 level 3 at compile time",
    "fused temporal D=24 threads=1024 natural", "fused temporal D=24 threads=1024 level 2 at compile time", "fused temporal D=24 threads=1024 level 3 at compile time",
    # msda_fused_tp_kernel<4, 4, 4, 32, 832, -1, 8> and <.., -1, 7>
    "fused temporal D=32 threads=832 8 waves", "fused temporal D=32 threads=832 7 waves",
}
NATIVE_BY_HAND = {
    # msda_fwd_kernel<VEC, 4, 4> and <VEC, 0, 0>
    "native v1 VEC=4 L4P4", "native v1 VEC=4 runtime L, P", "native v1 VEC=2 L4P4", "native v1 VEC=2 runtime L, P", "native v1 VEC=1 L4P4",
    "native v1 VEC=1 runtime L, P",
    # msda_fwd_v2_kernel<4, 4>, <2, 8>; msda_fwd_v3_kernel<4, 4, 1024>
    "native v2 L4P4", "native v2 L2P8", "native v3",
}


def test_case_lists_reach_every_dispatch_branch():
    fused, native = _launches()
    got = {r["inst"] for _, _, r in fused}
    assert got == FUSED_BY_HAND, (sorted(FUSED_BY_HAND - got), sorted(got - FUSED_BY_HAND))
    assert {r["inst"] for _, _, r in native} == NATIVE_BY_HAND
    assert len(FUSED_BY_HAND) == 4 + 24 + 21 + 20 and len(NATIVE_BY_HAND) == 9
    assert set(R.FUSED_INSTANCES) == FUSED_BY_HAND and set(R.NATIVE_INSTANCES) == NATIVE_BY_HAND      # (what the GPU file's launch table is checked against)

    def rows(s):
        H, W, _ = s["levels"]
        return [h * w for h, w in zip(H, W)]

    by = {}
    for n, sw, r in fused:
        if sw == R.DEFAULT_SWITCHES:
            by[n] = r
    # the encoder form at 150 KB: 911 staged rows fit beside the 1024-thread descriptors, 912 do not (LS rises by one)
    assert R.lds_bytes(911, 32, 1024) <= 150 * 1024 < R.lds_bytes(912, 32, 1024)
    a, b = by["enc 911|912 911 rows"], by["enc 911|912 912 rows"]
    assert (a["LS"], b["LS"]) == (1, 2) and a["inst"] == b["inst"] == "fused v3 D=32 threads=1024 natural"
    # two blocks per CU: 347 rows yes, 348 no; chunk 128 | 256 at 45 KB staged, 256 | 512 at 80 KB
    assert R.two_blocks_fit(R.lds_bytes(347, 32, 1024)) and not R.two_blocks_fit(R.lds_bytes(348, 32, 1024))
    assert by["enc two blocks 347 rows"]["two_blocks"] and not by["enc two blocks 348 rows"]["two_blocks"]
    assert (by["enc chunk 128|256 358 rows"]["chunk"], by["enc chunk 128|256 359 rows"]["chunk"]) == (128, 256)
    assert (by["enc chunk 256|512 638 rows"]["chunk"], by["enc chunk 256|512 639 rows"]["chunk"]) == (256, 512)
    # 72 KB of the decoder and temporal forms at every thread count
    for nt, lim in ((1024, 287), (832, 341), (512, 431)):
        assert R.lds_bytes(lim, 32, nt) <= 72 * 1024 < R.lds_bytes(lim + 1, 32, nt)
        for form in ("dec", "tp"):
            lo, hi = by[f"{form} 72 KB threads={nt} {lim} rows" if (form, nt) != ("tp", 1024) else "tp D=32 Q=128 LS=2"], by[f"{form} 72 KB threads={nt} {lim + 1} rows"]
            assert (lo["threads"], lo["LS"], hi["threads"], hi["LS"]) == (nt, 2, nt, 3), (form, nt, lo, hi)
    # thread counts and the even split into runs
    want = {1: (1, 512), 64: (64, 512), 65: (65, 832), 104: (104, 832), 105: (105, 1024), 128: (128, 1024), 129: (65, 832), 208: (104, 832), 209: (105, 1024)}
    for Q, (chunk, nt) in want.items():
        for form in ("dec", "tp"):
            r = by[f"{form} Q={Q}"]
            assert (r["chunk"], r["threads"]) == (chunk, nt) and r["LS"] == 1, (form, Q, r)
    # B on both sides of 16 with the XCD-aware order on and off, staged and gather
    for B in (1, 15, 16, 17):
        seen = {(sw["xcd_order"], r["inst"][:8]) for n, sw, r in fused if n == f"enc 40 B={B}"}
        assert seen == {(x, f) for x in (0, 1) for f in ("fused v2", "fused v3")}
    # forced budgets on the 40-token table: LS = 1, 2, 3 and nothing fits (the gather form)
    enc = [(sw, r) for n, sw, r in fused if n == "enc 40 D=32" and sw["variant"] == -1 and sw["stage_kb"] > 0]
    assert sorted((r["LS"] or 4) for _, r in enc) == [1, 2, 3, 4] and [r["inst"][:8] for sw, r in enc if sw["stage_kb"] == 36] == ["fused v2"]
    # D = 24: v2, the staged decoder form under a forced budget only, the temporal form
    d24 = [(sw, r) for n, sw, r in fused if n == "dec D=24 Q=104"]
    assert [r["inst"] for sw, r in d24 if sw == R.DEFAULT_SWITCHES] == ["fused v2 L4P4 map=0 waves hint=1 D=24"]
    assert "fused v3 D=24 threads=832 natural" in [r["inst"] for sw, r in d24]
    # the temporal form's fallbacks to v2
    for n in ("tp unlike pyramids", "tp Q=4097", "tp nothing fits"):
        assert by[n]["inst"] == "fused v2 L4P4 map=0 waves hint=1 D=32", n
    assert R.FUSED_SHAPES["tp Q=4097"]["Q"] == 4097 and by["tp Q=64"]["inst"].startswith("fused temporal")
    # the native op: S < 64, the budget's thresholds and its cap
    nat = {n: r for n, sw, r in native if sw == R.DEFAULT_SWITCHES}
    assert nat["v2 S = 63"]["inst"] == "native v2 L4P4" and nat["v3 S = 64"]["inst"] == "native v3"
    assert [nat[f"v3 budget {b}"]["budget"] for b in (358, 359, 638, 639, 959)] == [358, 359, 638, 639, 959]
    assert [nat[f"v3 budget {b}"]["chunk"] for b in (358, 359, 638, 639, 959)] == [128, 256, 256, 512, 512]
    assert nat["v3 budget capped at 960"]["budget"] == 960 and R.NATIVE_SHAPES["v3 budget capped at 960"]["S"] // 16 + 8 > 960
    assert {nat[n]["LS"] for n in nat if nat[n]["inst"] == "native v3"} >= {0, 1, 2, 4}
    assert nat["VEC=2 base at 8 bytes"]["inst"] == "native v1 VEC=2 L4P4" and nat["VEC=1 base at 4 bytes"]["inst"] == "native v1 VEC=1 L4P4"


def test_staged_form_is_refused_to_tables_that_are_not_one_run_of_tokens():
    """The staged fused kernel addresses level l at start[l] - start[LS] inside ONE staged run of tokens: the dispatcher's rule before
    this check existed (contiguity_rule=False: it counted H * W only) hands it the gapped and the descending table; the rule now does
    not.  A table whose staged levels [LS, L) are back to back stays staged, wherever the fine level lies."""
    for n in ("enc gap before level 3", "enc levels descending", "dec gap before level 2"):
        s = R.FUSED_SHAPES[n]
        old, new = R.msda_fused_branch(s, contiguity_rule=False), R.msda_fused_branch(s)
        assert old["inst"].startswith("fused v3") and old["LS"] == 1, (n, old)
        assert new["inst"].startswith("fused v2"), (n, new)
    s = R.FUSED_SHAPES["enc fine level last"]
    assert R.msda_fused_branch(s)["inst"].startswith("fused v3") and R.msda_fused_branch(s)["LS"] == 1
    for n, sw in R.FUSED_LAUNCHES:                       # every other table of the lists: the rule changes nothing
        if "gap" not in n and "descending" not in n:
            assert R.msda_fused_branch(R.FUSED_SHAPES[n], sw) == R.msda_fused_branch(R.FUSED_SHAPES[n], sw, contiguity_rule=False), n
