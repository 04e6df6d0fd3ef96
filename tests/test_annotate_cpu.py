"""The annotation pass (track boxes and captions on an overlay), the host side: the numpy reference (tests/_annotate_ref.py, a painter's
algorithm) against tiny pictures worked out by hand; the font; render.captions and render.ink on pinned examples; render.Style's new
fields and their refusals; the wrappers' refusals; the two ABI entries.  Integers only: every comparison is exact.  No GPU."""
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

import _annotate_ref as REF  # noqa: E402

ONE = (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E)                      # the glyph these pictures are worked out with


def _tables(texts):
    """A font that holds only '1' (= ONE) and '?' (a full block), a palette with row l = (10 l, 10 l + 1, 10 l + 2), ink row l = 200 + l."""
    font = np.zeros((64, 7), dtype=np.uint8)
    font[ord("1") - 32] = ONE
    font[ord("?") - 32] = 0x1F
    pal = np.array([[10 * l % 256, (10 * l + 1) % 256, (10 * l + 2) % 256] for l in range(256)], dtype=np.uint8)
    ink = np.array([[(200 + l) % 256] * 3 for l in range(256)], dtype=np.uint8)
    cap = np.zeros((256, 8), dtype=np.uint8)
    for l, text in texts.items():
        cap[l, :len(text)] = list(text)
    return pal, ink, cap, font


# ---- the reference against hand-worked pictures -----------------------------------------------------------------------------------------
def test_one_label_with_the_caption_1_at_scale_1_the_exact_ink_pixels():
    pal, ink, cap, font = _tables({1: b"1"})
    pic = np.full((1, 12, 16, 3), 7, dtype=np.uint8)
    geom = np.array([[4, 3, 10, 5, 11]])                               # the plate (7 x 9) sits above the box: columns 3..9, rows 1..9
    out = REF.annotate(pic, geom, 1, pal, ink, cap, font)
    inked = {(2, 6), (3, 5), (3, 6), (4, 6), (5, 6), (6, 6), (7, 6), (8, 5), (8, 6), (8, 7)}     # glyph row gy at Y = 2 + gy, pixel x at X = 4 + x
    for Y in range(12):
        for X in range(16):
            want = 7 if not (1 <= Y <= 9 and 3 <= X <= 9) else 201 if (Y, X) in inked else None
            assert out[0, Y, X].tolist() == ([want] * 3 if want is not None else [10, 11, 12]), (Y, X)
    # the box frame lies under it: box 1 around (3..5, 10..11) is all six of its pixels
    out = REF.annotate(pic, geom, 1, pal, ink, None, font, box=1)
    assert (out[0, 10:12, 3:6] == [10, 11, 12]).all() and int((out != 7).any(-1).sum()) == 6
    # at scale 2 the plate is 14 x 18: it no longer fits above the box (it starts at y0 = 10, its margin rows) nor right of x0 = 3 (px = 16 - 14)
    out = REF.annotate(pic, geom, 1, pal, ink, cap, font, scale=2)
    assert (out[0, :10] == 7).all() and (out[0, 10:12, 2:16] == [10, 11, 12]).all() and (out[0, 10:12, :2] == 7).all()


def test_a_plate_flips_inside_the_box_at_the_top_edge():
    pal, ink, cap, font = _tables({1: b"1"})
    pic = np.zeros((1, 14, 16, 3), dtype=np.uint8)
    out = REF.annotate(pic, np.array([[50, 2, 8, 12, 13]]), 1, pal, ink, cap, font)          # y0 - 9 = -1: inside, rows 8..13 of it
    touched = out.any(-1)[0]
    assert touched[8:14, 2:9].all() and int(touched.sum()) == 6 * 7
    assert out[0, 9, 5].tolist() == [201] * 3 and out[0, 10, 4].tolist() == [201] * 3 and out[0, 8, 5].tolist() == [10, 11, 12]
    out = REF.annotate(pic, np.array([[50, 2, 9, 12, 13]]), 1, pal, ink, cap, font)          # y0 - 9 = 0: above, rows 0..8
    touched = out.any(-1)[0]
    assert touched[0:9, 2:9].all() and int(touched.sum()) == 9 * 7


def test_a_plate_is_clamped_at_the_right_edge_and_clipped_when_wider_than_the_picture():
    pal, ink, cap, font = _tables({1: b"1", 2: b"1111"})
    pic = np.zeros((1, 20, 16, 3), dtype=np.uint8)
    out = REF.annotate(pic, np.array([[9, 13, 12, 15, 14]]), 1, pal, ink, cap, font)         # x0 = 13, w = 7: px = 16 - 7 = 9
    touched = out.any(-1)[0]
    assert touched[3:12, 9:16].all() and int(touched.sum()) == 63 and out[0, 4, 12].tolist() == [201] * 3
    geom = np.array([[0, 16, 20, -1, -1], [9, 5, 12, 15, 14]])                                # label 2: w = 25 > 16: px = 0, columns 16.. cut
    out = REF.annotate(pic, geom, 2, pal, ink, cap, font)
    touched = out.any(-1)[0]
    assert touched[3:12, :].all() and int(touched.sum()) == 9 * 16
    assert out[0, 4, 3].tolist() == [202] * 3 and out[0, 4, 9].tolist() == [202] * 3 and out[0, 4, 15].tolist() == [202] * 3


def test_the_priority_of_two_overlapping_labels():
    pal, ink, cap, font = _tables({1: b"1", 2: b"\x7f"})              # (0x7F is outside the font: drawn as '?', here a full block)
    pic = np.zeros((1, 24, 24, 3), dtype=np.uint8)
    geom = np.array([[30, 4, 10, 12, 20], [30, 6, 12, 20, 22]])        # plates: label 1 at (4..10, 1..9), label 2 at (6..12, 3..11)
    out = REF.annotate(pic, geom, 2, pal, ink, cap, font, box=2)
    assert out[0, 5, 8].tolist() == [10, 11, 12]                       # both plates hold it: label 1's (no ink of '1' there)
    assert out[0, 5, 7].tolist() == [201] * 3                          # ... and label 1's ink over label 2's ink
    assert out[0, 5, 11].tolist() == [202] * 3                         # label 2's alone: ink of its block
    assert out[0, 10, 11].tolist() == [202] * 3                        # label 2's plate over label 1's frame (row 10 is its top band)
    assert out[0, 11, 9].tolist() == [20, 21, 22]                      # ... its margin too
    assert out[0, 12, 5].tolist() == [10, 11, 12]                      # the frames: label 1's left band (columns 4..5) ...
    assert out[0, 13, 12].tolist() == [10, 11, 12]                     # ... and its right band over label 2's top band (rows 12..13)
    assert out[0, 12, 6].tolist() == [20, 21, 22] and out[0, 12, 8].tolist() == [20, 21, 22]    # label 1's interior is not drawn: label 2's frame shows
    assert out[0, 15, 8].tolist() == [0, 0, 0]                         # interior of both
    # a label below min_area, an empty row and rows that leave the picture draw nothing
    geom = np.array([[3, 4, 10, 12, 20], [0, 24, 24, -1, -1], [30, 4, 10, 24, 20], [30, -1, 10, 12, 20], [30, 4, 10, 12, 24], [30, 5, 4, 4, 9]])
    assert not REF.annotate(pic, geom, 6, pal, ink, cap, font, box=2, min_area=4).any()
    assert REF.annotate(pic, geom, 6, pal, ink, cap, font, box=2, min_area=3).any()


def test_surface_reference_chroma_rule_by_hand():
    pal, ink, cap, font = _tables({})
    pal = pal.astype(np.int64)
    pal[1] = (100, 40, 200)
    y = np.full((1, 5, 8), 9, dtype=np.uint8)                          # 5 x 7 picture, pitch 8
    uv = np.full((1, 3, 8), 0, dtype=np.uint8)
    uv[0, :, 0::2], uv[0, :, 1::2] = 60, 81
    oy, ouv = REF.annotate_yuv(y, uv, "nv12", 5, 7, np.array([[9, 1, 1, 6, 4]]), 1, pal, ink, None, font, box=1)
    assert oy[0, 1, 1:7].tolist() == [100] * 6 and oy[0, 4, 1:7].tolist() == [100] * 6 and oy[0, 2, 1] == 100 and oy[0, 2, 2] == 9
    assert (oy[0, :, 7] == 9).all() and (oy[0, 0] == 9).all()
    # pair (0, 0): one hit of four: (40 + 3 * 60 + 2) >> 2 = 55, (200 + 3 * 81 + 2) >> 2 = 111; pair (1, 1) (rows 2..3, columns 2..3): no hit
    assert ouv[0, 0, 0:2].tolist() == [55, 111] and ouv[0, 1, 2:4].tolist() == [60, 81]
    # pair (2, 3): row 4 only, column 6 only (the picture is 5 x 7): n = 1, the hit itself; pair (2, 0): columns 0..1 of row 4: (60 + 40 + 1) >> 1
    assert ouv[0, 2, 6:8].tolist() == [40, 200] and ouv[0, 2, 0:2].tolist() == [50, (81 + 200 + 1) >> 1]
    # P010: a written word is value << 6, an untouched one keeps its low bits
    y16 = np.full((1, 5, 8), (9 << 6) | 0x2A, dtype=np.uint16)
    uv16 = np.full((1, 3, 8), (60 << 6) | 0x15, dtype=np.uint16)
    oy, ouv = REF.annotate_yuv(y16, uv16, "p010", 5, 7, np.array([[9, 1, 1, 6, 4]]), 1, pal, ink, None, font, box=1)
    assert oy[0, 1, 1] == 100 << 6 and oy[0, 2, 2] == (9 << 6) | 0x2A and ouv[0, 1, 2] == (60 << 6) | 0x15
    assert ouv[0, 0, 0] == ((40 + 3 * 60 + 2) >> 2) << 6


# ---- the font ---------------------------------------------------------------------------------------------------------------------------
def test_font():
    from mdqe_cvpr2023_amd import render
    font = render.default_font()
    assert font.dtype == torch.uint8 and tuple(font.shape) == (64, 7)
    assert not bool(font[0].any())                                     # the space
    assert bool(font[1:].any(1).all()) and int(font.max()) < 32        # every other glyph shows something, in the low 5 bits
    assert len({tuple(g.tolist()) for g in font}) == 64                # pairwise distinct
    assert tuple(font[ord("1") - 32].tolist()) == ONE
    # every glyph uses both halves of its cell or is punctuation: letters and digits reach the top and the bottom row
    for ch in "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ":
        g = font[ord(ch) - 32]
        assert int(g[0]) and int(g[6]), ch


# ---- captions and ink -------------------------------------------------------------------------------------------------------------------
def _text(table, l):
    return bytes(table[l].tolist()).split(b"\0")[0].decode()


def test_captions_on_pinned_examples():
    from mdqe_cvpr2023_amd import render
    cls = torch.tensor([[0.1, 0.7, 0.7, 0.2], [0.995, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.004], [0.25, 0.5, 0.125, 0.0]], dtype=torch.float32)
    names = ("person", "Giant_Panda", "lizard", "a very long class name that does not fit")
    t = render.captions(render.Style(caption="id+class+score", class_names=names), cls, 4)
    assert t.dtype == torch.uint8 and tuple(t.shape) == (256, 32) and not t.is_cuda
    assert _text(t, 1) == "0 GIANT_PANDA 70%"                          # a tie: the first maximum; names upper-cased
    assert _text(t, 2) == "1 PERSON 100%"                              # 0.995 -> int(99.5 + 0.5)
    assert _text(t, 3) == "2 A VERY LONG CLASS NAME THAT DO" and len(_text(t, 3)) == 32          # cut at 32
    assert _text(t, 4) == "3 GIANT_PANDA 50%"
    assert not bool(t[0].any()) and not bool(t[5:].any())              # row 0 and the rows above n
    t = render.captions(render.Style(caption="class+score"), cls, 3)
    assert [_text(t, l) for l in range(1, 5)] == ["1 70%", "0 100%", "3 0%", ""]                # without names the class id; 0.004 -> "0%"
    assert [_text(render.captions(render.Style(caption="class"), cls, 4), l) for l in (1, 4)] == ["1", "1"]
    assert [_text(render.captions(render.Style(caption="id+class", class_names=names), cls, 2), l) for l in (1, 2, 3)] == ["0 GIANT_PANDA", "1 PERSON", ""]
    t = render.captions(render.Style(caption="id"), None, 255)        # ids alone need no class rows
    assert _text(t, 1) == "0" and _text(t, 255) == "254" and _text(t, 0) == ""
    assert not bool(render.captions(render.Style(), cls, 4).any()) and not bool(render.captions(render.Style(caption="id"), cls, 0).any())
    again = render.captions(render.Style(caption="id+class+score", class_names=names), cls.clone(), 4)
    assert torch.equal(again, render.captions(render.Style(caption="id+class+score", class_names=names), cls, 4))      # a pure function
    with pytest.raises(ValueError, match="needs the window's class rows"):
        render.captions(render.Style(caption="class"), None, 2)
    with pytest.raises(ValueError, match="needs the window's class rows"):
        render.captions(render.Style(caption="id+class"), cls[:1], 2)


def test_ink():
    from mdqe_cvpr2023_amd import render
    pal = torch.zeros(256, 3, dtype=torch.uint8)
    pal[1] = torch.tensor([127, 128, 128])                             # 383: dark
    pal[2] = torch.tensor([128, 128, 128])                             # 384: light
    pal[3] = torch.tensor([255, 255, 255])
    pal[4] = torch.tensor([255, 0, 128])
    ink = render.ink(pal)
    assert ink.dtype == torch.uint8 and tuple(ink.shape) == (256, 3) and ink.is_contiguous()
    assert ink[:5].tolist() == [[255] * 3, [255] * 3, [0] * 3, [0] * 3, [255] * 3]
    d = render.ink(render.default_palette())
    assert set(d.unique().tolist()) == {0, 255} and bool((d[:, 0] == d[:, 1]).all()) and bool((d[:, 1] == d[:, 2]).all())
    for fmt, white, black, mid in (("nv12", 235, 16, 128), ("p010", 940, 64, 512)):           # order-independent on a surface
        a, b = (render.palette_yuv(d, fmt, "bt709", False, order).to(torch.int32) for order in ("rgb", "bgr"))
        assert torch.equal(a, b) and set(a[:, 0].tolist()) == {white, black} and bool((a[:, 1:] == mid).all())
    with pytest.raises(ValueError, match="ink: palette must be"):
        render.ink(pal[:255])


# ---- the style --------------------------------------------------------------------------------------------------------------------------
def test_style_fields_their_defaults_and_every_refusal():
    from mdqe_cvpr2023_amd.render import Style
    st = Style()
    assert (st.box, st.caption, st.class_names, st.text_scale, st.min_area) == (0, None, None, 1, 0) and st.annotates is False
    assert Style(box=1).annotates is True and Style(caption="id").annotates is True and Style(text_scale=3, min_area=50).annotates is False
    for cap in (None, "id", "class", "id+class", "id+class+score", "class+score"):
        assert Style(caption=cap).caption == cap
    assert Style(class_names=["a", "b"]).class_names == ("a", "b")
    for kw, what in (({"box": -1}, "box"), ({"box": 5}, "box"), ({"box": True}, "box"), ({"box": 1.0}, "box"),
                     ({"caption": "score"}, "caption"), ({"caption": "class+id"}, "caption"), ({"caption": ""}, "caption"), ({"caption": 1}, "caption"),
                     ({"class_names": "person"}, "class_names"), ({"class_names": [1, 2]}, "class_names"), ({"class_names": 3}, "class_names"),
                     ({"text_scale": 0}, "text_scale"), ({"text_scale": 5}, "text_scale"), ({"text_scale": 2.0}, "text_scale"),
                     ({"text_scale": True}, "text_scale"), ({"min_area": -1}, "min_area"), ({"min_area": 0.5}, "min_area"),
                     ({"min_area": 2 ** 31}, "min_area"), ({"min_area": False}, "min_area")):
        with pytest.raises(ValueError, match="overlay style: %s must be" % what):
            Style(**kw)
    # the cached host-made tables (on the CPU "device" here), and the captions of a window
    st = Style(box=2, caption="id")
    assert st.font_on("cpu") is st.font_on("cpu") and st.ink_on("cpu") is st.ink_on("cpu")
    assert tuple(st.font_on("cpu").shape) == (64, 7) and tuple(st.ink_on("cpu").shape) == (256, 3)
    y = st.ink_yuv_on("cpu", "nv12", "bt601", True, "bgr")
    assert y is st.ink_yuv_on("cpu", "nv12", "bt601", True, "bgr") and y.dtype == torch.uint16 and tuple(y.shape) == (256, 3)
    assert tuple(st.captions_on("cpu", None, 3).shape) == (256, 32) and Style(box=1).captions_on("cpu", None, 3) is None


def test_wrappers_refuse_bad_arguments_before_they_look_at_devices():
    from mdqe_cvpr2023_amd import ops, render
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    pal = render.default_palette()
    ink, font = render.ink(pal), render.default_font()
    cap = torch.zeros(256, 32, dtype=torch.uint8)
    pic = torch.zeros(2, 6, 9, 3, dtype=torch.uint8)
    geom = torch.zeros(3 * 2, 5, dtype=torch.int32)
    ok = dict(pic=pic, geom=geom, n=3, palette=pal, ink=ink, captions=cap, font=font)
    for kw, what in (({"n": 256}, "n must be"), ({"n": -1}, "n must be"), ({"box": 5}, "box must be"), ({"scale": 0}, "scale must be"),
                     ({"scale": 5}, "scale must be"), ({"min_area": -1}, "min_area must be"), ({"f_off": -1}, "f_off must be"),
                     ({"geom": geom.float()}, "geom must be"), ({"geom": geom[:5]}, "geom must be"), ({"geom": geom.view(2, 3, 5)}, "geom must be"),
                     ({"palette": pal[:255]}, "palette must be"), ({"ink": ink.float()}, "ink must be"),
                     ({"captions": cap[:255]}, "captions must be"), ({"captions": torch.zeros(256, 65, dtype=torch.uint8)}, "captions must be"),
                     ({"font": font[:63]}, "font must be"), ({"pic": pic[..., :2]}, "pic must be"), ({"pic": pic.float()}, "pic must be"),
                     ({"f_off": 1}, "must hold frames"), ({}, "must be a CUDA tensor on pic's device")):
        with pytest.raises(RuntimeError, match="annotate: .*" + what):
            ops.annotate(**dict(ok, **kw))
    s = YuvFrames.empty(2, 6, 9)
    py = render.palette_yuv(pal, "nv12", "bt709", False, "rgb")
    iy = render.palette_yuv(ink, "nv12", "bt709", False, "rgb")
    with pytest.raises(RuntimeError, match="annotate_yuv: yuv must be a preprocess.YuvFrames"):
        ops.annotate_yuv(pic, geom, 3, py, iy, cap, font)
    with pytest.raises(RuntimeError, match="annotate_yuv: palette must be contiguous uint16"):
        ops.annotate_yuv(s, geom, 3, pal, iy, cap, font)
    with pytest.raises(RuntimeError, match="annotate_yuv: yuv holds 2 surfaces"):
        ops.annotate_yuv(s, geom, 3, py, iy, cap, font, 1)
    with pytest.raises(RuntimeError, match="annotate_yuv: the surfaces must be on a HIP device"):
        ops.annotate_yuv(s, geom, 3, py, iy, cap, font)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_both_entries():
    from mdqe_cvpr2023_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    for name, n_args in (("mdqe_annotate_u8", 16), ("mdqe_annotate_yuv420sp", 22)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
        assert hasattr(h, name) and name in _lib.SIGNATURES
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == n_args
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # new entries only
