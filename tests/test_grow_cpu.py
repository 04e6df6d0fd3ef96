"""The redaction margin, the host side: the two numpy forms of the rule (tests/_grow_ref.py) against each other and against known answers;
render.Style's `grow` field and its `grows` table; the ABI entry's refusals, called through the library; ops.grow_labels' argument
checks; and the launches merge.overlay_frames makes, with the ops replaced by recorders.  Integers only: every comparison is exact.
No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _grow_ref as REF  # noqa: E402

RADII = (0, 1, 2, 5, 17, 32)


def _table(*labels):
    t = np.zeros(256, dtype=np.uint8)
    t[list(labels)] = 1
    return t


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 3), (3, 40), (23, 31)])
def test_the_two_reference_forms_agree(size):
    H, W = size
    rng = np.random.default_rng(H * 100 + W)
    for radius in RADII:
        # sparse maps (a few labels on a background) and dense ones, with random tables
        sparse = np.where(rng.random((2, H, W)) < 0.04, rng.integers(1, 6, size=(2, H, W)), 0).astype(np.uint8)
        dense = rng.integers(0, 4, size=(2, H, W)).astype(np.uint8)
        for lab in (sparse, dense):
            table = rng.integers(0, 2, size=256).astype(np.uint8)
            a, b = REF.grow(lab, table, radius), REF.grow_pixelwise(lab, table, radius)
            assert a.dtype == np.uint8 and np.array_equal(a, b), (size, radius)
            if radius == 0:
                assert np.array_equal(a, lab)
            g = REF.growing(table)
            assert np.array_equal(a[g[lab]], lab[g[lab]])             # a growing region is never overwritten
        assert np.array_equal(REF.grow(dense, np.zeros(256, dtype=np.uint8), radius), dense)     # no growing label: a copy
        assert np.array_equal(REF.grow(dense, _table(0), radius), dense)                          # entry 0 is ignored


def test_known_answers():
    one = np.zeros((1, 21, 21), dtype=np.uint8)
    one[0, 10, 10] = 9
    for radius, count in ((0, 1), (1, 5), (2, 13), (3, 29), (5, 81)):
        for fn in (REF.grow, REF.grow_pixelwise):
            out = fn(one, _table(9), radius)
            assert int((out == 9).sum()) == count and int((out != 0).sum()) == count, (radius, fn.__name__)
    # offset (3, 4) is at distance 5 exactly and is taken at radius 5; (4, 4) is not
    out = REF.grow(one, _table(9), 5)
    assert out[0, 13, 14] == 9 and out[0, 7, 6] == 9 and out[0, 14, 14] == 0 and out[0, 6, 6] == 0
    assert out[0, 10, 15] == 9 and out[0, 10, 16] == 0
    # labels 7 and 3 at equal distance give 3: a horizontal, a vertical and a mixed tie ((0, 5) against (3, 4))
    for p7, p3, at in (((5, 2), (5, 8), (5, 5)), ((2, 5), (8, 5), (5, 5)), ((5, 10), (8, 9), (5, 5)), ((8, 9), (5, 10), (5, 5))):
        for a, b in ((7, 3), (3, 7)):                                 # (whichever comes first in scan order)
            lab = np.zeros((1, 12, 12), dtype=np.uint8)
            lab[0][p7], lab[0][p3] = a, b
            for fn in (REF.grow, REF.grow_pixelwise):
                assert fn(lab, _table(3, 7), 5)[0][at] == 3, (p7, p3, a, b)
    # the nearer label wins whatever its number
    lab = np.zeros((1, 1, 9), dtype=np.uint8)
    lab[0, 0, 0], lab[0, 0, 8] = 3, 7
    assert REF.grow(lab, _table(3, 7), 8)[0, 0].tolist() == [3, 3, 3, 3, 3, 7, 7, 7, 7]
    # a growing label is never overwritten, a track that does not grow is, and alone it stays
    lab = np.zeros((1, 5, 9), dtype=np.uint8)
    lab[0, :, :3], lab[0, :, 3:6], lab[0, :, 6:] = 4, 5, 6
    out = REF.grow(lab, _table(4, 6), 2)
    assert out[0, 2].tolist() == [4, 4, 4, 4, 4, 6, 6, 6, 6]          # (column 4: distance 2 to label 4, 2 to label 6: the smaller label)
    assert np.array_equal(REF.grow(lab, _table(5), 1)[0, 2], [4, 4, 5, 5, 5, 5, 5, 6, 6])
    assert np.array_equal(REF.grow(lab, _table(9), 32), lab)
    # nothing is read beyond the border: a blob in a corner grows into the picture only, and the shape is kept
    lab = np.zeros((2, 4, 6), dtype=np.uint8)
    lab[1, 0, 0] = 1
    out = REF.grow(lab, _table(1), 2)
    assert not out[0].any() and out[1].tolist() == [[1, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0] * 6]


# ---- render.Style --------------------------------------------------------------------------------------------------------------------
def test_style_grow_validation_and_the_grows_table():
    from mdqe_cvpr2023_amd.render import Style
    assert Style().grow == 0 and Style() == Style(grow=0) and Style(grow=32).grow == 32 and Style(blur="tracks", grow=4).grow == 4
    for bad in (True, False, 4.0, -1, 33, "4", None):
        with pytest.raises(ValueError, match="grow must be an int in 0..32"):
            Style(grow=bad)
    for what in ("tracks", "background"):
        with pytest.raises(ValueError, match="(?s)grow.*matte_gain"):
            Style(replace=what, grow=1)
        assert Style(replace=what, grow=0).grow == 0
    every = [0] + [1] * 255
    for kw in ({}, {"mosaic": "background"}, {"blur": "background"}, {"mosaic": "tracks"}, {"blur": "tracks"}, {"alpha": 0.25, "contour": 0}):
        st = Style(grow=3, **kw)
        g = st.grows()
        assert g.dtype == torch.uint8 and tuple(g.shape) == (256,) and not g.is_cuda and g.tolist() == every, kw
        assert Style(**kw).grows().tolist() == every                  # (the table does not depend on the margin)
    rows = torch.tensor([[0.1, 0.9, 0.2, 0.0],       # class 1
                         [0.5, 0.1, 0.5, 0.3],       # a tie of 0 and 2: class 0
                         [0.0, 0.2, 0.7, 0.7],       # a tie of 2 and 3: class 2
                         [0.0, 0.0, 0.0, 0.6]])      # class 3
    for kw, r in (({"mosaic": "tracks"}, 2), ({"blur": "tracks"}, 3)):
        for classes in ([2], [0, 3], [1, 2, 3], [9]):
            st = Style(grow=5, classes=classes, **kw)
            act = st.actions(rows)
            want = (act == r).to(torch.uint8)
            assert st.grows(rows).tolist() == want.tolist() and int(want[0]) == 0 and int(want[5:].sum()) == 0
            assert st.grows(rows)[1:5].tolist() == [int(c in classes) for c in (1, 0, 2, 3)]
        assert Style(grow=5, classes=[1], **kw).grows(torch.zeros(0, 4)).tolist() == [0] * 256
        with pytest.raises(ValueError, match="class rows"):
            Style(grow=5, classes=[1], **kw).grows()
    # the device tables: cached per device unless the table depends on the window
    st = Style(blur="tracks", grow=2)
    assert st.grows_on("cpu") is st.grows_on("cpu") and st.grows_on("cpu").tolist() == every
    st = Style(blur="tracks", grow=2, classes=[0])
    a, b = st.grows_on("cpu", rows), st.grows_on("cpu", rows[:1])
    assert a.tolist() == [0, 0, 1, 0, 0] + [0] * 251 and b.tolist() == [0] * 256


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_entry_and_it_refuses_bad_arguments():
    from mdqe_cvpr2023_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    name = "mdqe_grow_labels_u8"
    assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
    assert hasattr(h, name) and name in _lib.SIGNATURES
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == 8
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # a new entry only
    EINVAL = 1

    def call(F=1, Ho=8, Wo=8, radius=4, labels=None, grow=None, out=None):
        return h.mdqe_grow_labels_u8(labels, F, Ho, Wo, grow, radius, out, None)
    for kw in ({"radius": -1}, {"radius": 33}, {"F": -1}, {"Ho": -1}, {"Wo": -1}, {"F": 1 << 16, "Ho": 1 << 8, "Wo": 1 << 8}):
        assert call(**kw) == EINVAL, kw
        if "F" not in kw:
            assert call(**dict(kw, F=0)) == EINVAL, kw                # ... whatever F says
    for radius in (0, 1, 32):
        assert call(F=0, radius=radius) == 0 and call(Ho=0, radius=radius) == 0 and call(Wo=0, radius=radius) == 0      # OK, nothing launched
    assert call() == EINVAL                                           # null pointers with something to do
    # never dereferenced (the refusals come before the launch): a missing pointer, and an out that meets labels or the table
    ptrs = {"labels": 1 << 20, "grow": 2 << 20, "out": 3 << 20}
    for missing in ptrs:
        assert call(**dict(ptrs, **{missing: None})) == EINVAL, missing
    for kw in ({"out": ptrs["labels"]}, {"out": ptrs["labels"] + 63}, {"out": ptrs["labels"] - 63}, {"out": ptrs["grow"] + 255},
               {"out": ptrs["grow"] - 63}, {"labels": ptrs["out"] + 1}, {"grow": ptrs["out"] + 63}):
        assert call(**dict(ptrs, **kw)) == EINVAL, kw


def test_wrapper_argument_checks():
    from mdqe_cvpr2023_amd import ops
    lab = torch.zeros(2, 6, 9, dtype=torch.uint8)
    table = torch.ones(256, dtype=torch.uint8)
    for bad in (lab.float(), lab[0], lab[:, :, ::2], None, lab.numpy()):
        with pytest.raises(RuntimeError, match="grow_labels: labels must be contiguous uint8 .F, Ho, Wo."):
            ops.grow_labels(bad, table, 4)
    for bad in (table.float(), table[:255], torch.ones(512, dtype=torch.uint8)[::2], table.view(1, 256), None, table.tolist()):
        with pytest.raises(RuntimeError, match="grow_labels: grow must be contiguous uint8 .256."):
            ops.grow_labels(lab, bad, 4)
    for bad in (-1, 33, 4.0, True, None):
        with pytest.raises(RuntimeError, match="grow_labels: radius must be an int in 0..32"):
            ops.grow_labels(lab, table, bad)
    for bad in (lab[:1].clone(), lab.float(), torch.zeros(2, 6, 18, dtype=torch.uint8)[:, :, ::2], lab.numpy()):
        with pytest.raises(RuntimeError, match="grow_labels: out must be contiguous uint8"):
            ops.grow_labels(lab, table, 4, bad)
    # shapes and dtypes first, devices after: a host without a GPU gets as far as the device check
    with pytest.raises(RuntimeError, match="grow_labels: labels must be a CUDA tensor"):
        ops.grow_labels(lab, table, 4)


# ---- merge.overlay_frames: which launches a style makes ---------------------------------------------------------------------------------
class _Store:
    """A FrameStore's `pieces` for frames [10, 15): two pieces of 3 and 2 frames."""
    def __init__(self, make):
        self.make = make

    def pieces(self, f0, f1, stream=None):
        assert (f0, f1) == (10, 15)
        return [(self.make(3), 10), (self.make(2), 13)]


PAINTERS = ("render_overlay", "render_overlay_yuv", "render_mosaic", "render_mosaic_yuv", "render_blur", "render_blur_yuv")


def _record(monkeypatch, style, surface, n=2):
    """The (name, args) of every ops call merge.overlay_frames makes for one window of 5 frames of 6 x 8 and n tracks; ops.grow_labels is
    replaced by the numpy rule."""
    from mdqe_cvpr2023_amd import merge, ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    calls = []
    for name in PAINTERS + ("annotate", "annotate_yuv", "render_trails", "render_trails_yuv"):
        monkeypatch.setattr(ops, name, (lambda n: lambda *a, **kw: calls.append((n, a, kw)))(name))

    def grow_labels(labels, table, radius, out=None):
        calls.append(("grow_labels", (labels, table, radius, out), {}))
        assert out is not None and out.shape == labels.shape and out.dtype == torch.uint8
        out.copy_(torch.from_numpy(REF.grow(labels.numpy(), table.numpy(), radius)))
        return out
    monkeypatch.setattr(ops, "grow_labels", grow_labels)
    monkeypatch.setattr(merge, "label_maps", lambda *a: torch.zeros(n, 5, 5, dtype=torch.int32))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    m = torch.zeros(n, 5, 3, 4)
    labels = torch.zeros(7, 6, 8, dtype=torch.uint8)
    labels[:, 2, 2], labels[:, 4, 6] = 1, 2
    before = labels.clone()
    if surface:
        out = YuvFrames.empty(6, 6, 8, fmt="nv12", matrix="bt601", full_range=True, order="bgr")
        store = _Store(lambda k: YuvFrames.empty(k, 6, 8, fmt="nv12", matrix="bt601", full_range=True, order="bgr"))
    else:
        out = torch.zeros(6, 6, 8, 3, dtype=torch.uint8)
        store = _Store(lambda k: torch.zeros(k, 3, 6, 8, dtype=torch.uint8))
    cls = torch.tensor([[0.9, 0.1], [0.2, 0.8]])[:n]
    assert merge.overlay_frames(m, 8, (6, 8), (6, 8), False, labels, 1, store, 10, style, cls, out, 1) is None
    assert torch.equal(labels, before)                                # the window's label map keeps its bits
    return calls, labels, out


@pytest.mark.parametrize("surface", [False, True])
def test_overlay_frames_grows_behind_the_label_map_and_hands_the_painters_the_grown_map(monkeypatch, surface):
    from mdqe_cvpr2023_amd.render import Style
    sfx = "_yuv" if surface else ""
    # grow == 0: exactly the former calls, with the label map's own frames
    for st, painter in ((Style(), "render_overlay"), (Style(mosaic="tracks"), "render_mosaic"), (Style(blur="tracks"), "render_blur")):
        calls, labels, _ = _record(monkeypatch, st, surface)
        assert [c[0] for c in calls] == [painter + sfx] * 2
        for (_, a, _), (l0, k) in zip(calls, ((1, 3), (4, 2))):
            assert torch.equal(a[0], labels[l0:l0 + k]) and a[0].data_ptr() == labels[l0:l0 + k].data_ptr()
    # grow > 0: one grow launch over the window's frames, then the painters on the grown map's pieces
    for st, painter, table in ((Style(grow=1), "render_overlay", [0] + [1] * 255), (Style(mosaic="background", grow=2), "render_mosaic", [0] + [1] * 255),
                               (Style(blur="tracks", grow=1), "render_blur", [0] + [1] * 255),
                               (Style(blur="tracks", classes=[1], grow=2), "render_blur", [0, 0, 1] + [0] * 253),
                               (Style(mosaic="tracks", classes=[0], grow=1, box=1, caption="id", trail=0), "render_mosaic", [0, 1, 0] + [0] * 253)):
        calls, labels, out = _record(monkeypatch, st, surface)
        tail = ["annotate" + sfx] * 2 if st.annotates else []
        assert [c[0] for c in calls] == ["grow_labels"] + [painter + sfx] * 2 + tail, st
        lab, tab, radius, scratch = calls[0][1]
        assert torch.equal(lab, labels[1:6]) and lab.data_ptr() == labels[1:6].data_ptr() and tab.tolist() == table and radius == st.grow
        assert scratch is not None and tuple(scratch.shape) == (5, 6, 8) and scratch.is_contiguous()
        want = torch.from_numpy(REF.grow(labels[1:6].numpy(), np.array(table, dtype=np.uint8), st.grow))
        assert not torch.equal(want, labels[1:6])
        for (_, a, _), (d, k) in zip(calls[1:3], ((0, 3), (3, 2))):
            assert torch.equal(a[0], want[d:d + k]) and a[0].data_ptr() == scratch[d:d + k].data_ptr() and len(a[1]) == k
        if st.classes is None:
            assert tab is st.grows_on("cpu")                          # the cached table
    # a window without tracks: nothing grows, nothing is allocated
    calls, labels, _ = _record(monkeypatch, Style(blur="tracks", grow=4), surface, n=0)
    assert [c[0] for c in calls] == ["render_blur" + sfx] * 2
