"""Decoder surfaces as video input, the host side: the integer rule against float64 and Pillow (these two validate the ORACLE,
tests/_yuv_ref.py, and the rule itself -- they run no package code; the package is tied to the oracle by the table test and by the exact
CPU and GPU comparisons), the package's table against the header's and the reference's own derivation, the CPU restatement of the rule (preprocess.yuv_to_rgb on host planes) against the numpy
oracle over the shape list of the GPU tests, YuvFrames' validation / views / slicing, and the ABI entry's refusals.  No GPU."""
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

import _yuv_ref as REF  # noqa: E402

# the issue's table, typed in: (matrix, full_range, bits) -> yo, co, cy, rv, gu, gv, bu
TABLE = {
    ("bt601", False, 8): (16, 128, 76309, 104597, -25675, -53279, 132201),
    ("bt601", True, 8): (0, 128, 65536, 91881, -22553, -46802, 116130),
    ("bt709", False, 8): (16, 128, 76309, 117489, -13975, -34925, 138438),
    ("bt709", True, 8): (0, 128, 65536, 103206, -12276, -30679, 121609),
    ("bt601", False, 10): (64, 512, 19077, 26149, -6419, -13320, 33050),
    ("bt601", True, 10): (0, 512, 16336, 22903, -5622, -11666, 28947),
    ("bt709", False, 10): (64, 512, 19077, 29372, -3494, -8731, 34610),
    ("bt709", True, 10): (0, 512, 16336, 25726, -3060, -7647, 30313),
}
SHAPES = [(1, 1), (2, 2), (1, 33), (19, 37), (32, 64), (33, 131), (64, 1040)]
BITS = {"nv12": 8, "p010": 10}


def _header():
    return open(os.path.join(ROOT, "include", "mdqe_hip.h")).read()


def test_the_table_is_the_same_everywhere():
    from mdqe_cvpr2023_amd import preprocess as P
    assert len(P.YUV_COEFFS) == 8
    for (matrix, full, bits), row in TABLE.items():
        fmt = "nv12" if bits == 8 else "p010"
        assert REF.coeffs(matrix, full, bits) == row, (matrix, full, bits)
        assert P.YUV_COEFFS[(fmt, matrix, full)] == row
    # the header's macro, row = 4 * fmt + 2 * matrix + full_range
    body = re.search(r"#define\s+MDQE_YUV_COEFFS\s*\{(.*?)\n\s*int\s+mdqe_yuv420sp_to_rgb_u8", _header(), flags=re.S).group(1)
    rows = [tuple(int(v) for v in re.findall(r"-?\d+", r)) for r in re.findall(r"\{([^{}]*)\}", re.sub(r"/\*.*?\*/", "", body, flags=re.S))]
    assert len(rows) == 8
    for k, row in enumerate(rows):
        fmt, matrix, full = P.YUV_FORMATS[k // 4], P.YUV_MATRICES[(k // 2) % 2], bool(k % 2)
        assert row == P.YUV_COEFFS[(fmt, matrix, full)], k


@pytest.mark.parametrize("matrix,full,bits", sorted(TABLE))
def test_rule_against_float64(matrix, full, bits):
    """(Validates the oracle's rule, not package code.)  All (Y, U, V) for 8 bits, every 5th value (and the top one) for 10: within 1 level of clamp(rint(float64)), equal on greys in
    full range, and the accumulator far inside int32.  How often an output differs from the rounded float64 value at all is printed,
    not asserted: at most 0.05 % of the outputs of a channel for 8 bits and 0.19 % for 10 (a constant rounded to 1/65536 is
    multiplied by a sample four times as large); counted per TRIPLE, any channel, at most 0.09 % and 0.37 %."""
    ax = np.arange(256) if bits == 8 else np.unique(np.concatenate([np.arange(0, 1024, 5), [1023]]))
    Y, U, V = np.meshgrid(ax, ax, ax, indexing="ij", sparse=True)
    got, acc = REF.rule(Y, U, V, matrix, full, bits)
    want = REF.float_rule(Y, U, V, matrix, full, bits)
    # the largest accumulator in closed form: full-scale luma plus the largest chroma term (|u|, |v| <= co) plus the rounding constant --
    # 36.1e6 at most (BT.709 limited 10-bit, B), a sixtieth of what int32 holds
    yo, co, cy, rv, gu, gv, bu = TABLE[(matrix, full, bits)]
    bound = ((1 << bits) - 1 - yo) * cy + max(abs(rv), abs(gu) + abs(gv), abs(bu)) * co + 32768
    assert acc <= bound < 3.7e7 < 2 ** 31 / 32
    shape = np.broadcast_shapes(Y.shape, U.shape, V.shape)
    differ, per_output = np.zeros(shape, dtype=bool), []
    for g, w in zip(got, want):
        d = np.abs(g - w)
        assert int(d.max()) <= 1
        differ |= np.broadcast_to(d != 0, shape)
        per_output.append(100.0 * float(np.broadcast_to(d != 0, shape).mean()))
    print(matrix, full, bits, "max |acc| %d; differ from rint(float64): R %.4f %% G %.4f %% B %.4f %% of the outputs, %.4f %% of the triples"
          % ((acc,) + tuple(per_output) + (100.0 * differ.mean(),)))
    if full:
        co = 128 << (bits - 8)
        grey, _ = REF.rule(ax, co, co, matrix, full, bits)
        fg = REF.float_rule(ax, co, co, matrix, full, bits)
        assert all(np.array_equal(g, w) for g, w in zip(grey, fg))
        assert all(np.array_equal(g, grey[0]) for g in grey)


def test_full_range_bt601_against_pillow():
    """(Validates the oracle's rule, not package code.)  All 2^24 triples within 1 level of Pillow's own YCbCr -> RGB."""
    from PIL import Image
    ax = np.arange(256)
    worst = 0
    for y0 in range(0, 256, 16):                                      # 16 images of 16 x 65536 pixels: all (Y, U, V)
        Y, U, V = np.meshgrid(ax[y0:y0 + 16], ax, ax, indexing="ij")
        ycc = np.stack([Y, U, V], -1).reshape(16, 65536, 3).astype(np.uint8)
        pil = np.asarray(Image.fromarray(ycc, "YCbCr").convert("RGB")).astype(np.int64)
        (R, G, B), _ = REF.rule(Y, U, V, "bt601", True, 8)
        got = np.stack([R, G, B], -1).reshape(16, 65536, 3)
        worst = max(worst, int(np.abs(got - pil).max()))
    assert worst <= 1


def _host_frames(seed, n, H, W, fmt, pitch, chroma_row, extra_rows=0, lead=0, **kw):
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    ys, cs = REF.make_content(seed, n, H, W, fmt)
    flat, rows = REF.pack(ys, cs, fmt, pitch, chroma_row, extra_rows, lead)
    y, uv = REF.plane_views(torch.from_numpy(flat), n, H, W, fmt, pitch, chroma_row, rows, lead)
    return YuvFrames(y, uv, H, W, fmt=fmt, **kw), ys, cs, flat


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_cpu_conversion_equals_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd.preprocess import yuv_to_rgb
    tight = REF.tight_pitch(W, fmt)
    k = 0
    for matrix in ("bt601", "bt709"):
        for full in (False, True):
            for order in ("rgb", "bgr"):
                pitch = (tight, (tight + 255) // 256 * 256, tight + (1 if fmt == "nv12" else 2))[k % 3]
                crow = (H, (H + 31) // 32 * 32)[k % 2]
                s, ys, cs, flat = _host_frames(H * 1000 + W, 2, H, W, fmt, pitch, crow, extra_rows=k % 4, lead=(k % 2) * (1 if fmt == "nv12" else 2),
                                               matrix=matrix, full_range=full, order=order)
                before = flat.copy()
                got = yuv_to_rgb(s)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, H, W) and got.is_contiguous() and not got.is_cuda
                assert np.array_equal(got.numpy(), REF.convert(ys, cs, H, W, fmt, matrix, full, order)), (matrix, full, order, pitch, crow)
                assert np.array_equal(flat, before)
                k += 1


def test_p010_ignores_the_low_six_bits_and_takes_both_word_types():
    from mdqe_cvpr2023_amd.preprocess import YuvFrames, yuv_to_rgb
    ys, cs = REF.make_content(5, 1, 6, 10, "p010")
    a = yuv_to_rgb(YuvFrames(torch.from_numpy(ys.view(np.int16)), torch.from_numpy(cs.view(np.int16)), 6, 10, fmt="p010"))
    b = yuv_to_rgb(YuvFrames(torch.from_numpy(ys.view(np.int16)).view(torch.uint16), torch.from_numpy(cs.view(np.int16)).view(torch.uint16), 6, 10, fmt="p010"))
    c = yuv_to_rgb(YuvFrames(torch.from_numpy((ys & 0xFFC0).view(np.int16)), torch.from_numpy((cs | 0x3F).view(np.int16)), 6, 10, fmt="p010"))
    assert torch.equal(a, b) and torch.equal(a, c)
    assert int((ys & 0x3F).max()) > 0 and int((ys >> 6).max()) > 511           # (low bits set; words with the sign bit of int16 set)


def test_yuvframes_validation():
    from mdqe_cvpr2023_amd.preprocess import YuvFrames, yuv_to_rgb
    y, uv = torch.zeros(2, 6, 16, dtype=torch.uint8), torch.zeros(2, 3, 16, dtype=torch.uint8)
    s = YuvFrames(y, uv, 5, 9)
    assert (len(s), s.height, s.width, s.fmt, s.matrix, s.full_range, s.order) == (2, 5, 9, "nv12", "bt709", False, "rgb")
    YuvFrames(y, uv, 6, 16)
    YuvFrames(y[:, :, :1], uv[:, :, :2], 6, 1)
    for kw, name in (({"fmt": "i420"}, "fmt"), ({"matrix": "bt2020"}, "matrix"), ({"order": "gbr"}, "order"), ({"full_range": 1}, "full_range")):
        with pytest.raises(ValueError, match=name):
            YuvFrames(y, uv, 5, 9, **kw)
    for h, w, name in ((0, 9, "height"), (5, 0, "width"), (5.0, 9, "height"), (5, True, "width"), (-1, 9, "height")):
        with pytest.raises(ValueError, match=name):
            YuvFrames(y, uv, h, w)
    for h, w in ((7, 9), (5, 17)):
        with pytest.raises(ValueError, match="y holds"):
            YuvFrames(y, uv, h, w)
    with pytest.raises(ValueError, match="uv holds"):
        YuvFrames(y, uv[:, :2], 5, 9)
    with pytest.raises(ValueError, match="uv holds"):
        YuvFrames(y, uv[:, :, :9], 5, 9)                              # 9 pixels need 5 pairs = 10 samples
    with pytest.raises(ValueError, match="uv holds 1 surfaces"):
        YuvFrames(y, uv[:1], 5, 9)
    for bad, name in ((y.float(), "y must be torch.uint8"), (y[0], r"y must be a \[n, rows, pitch\]"), (y[:, :, ::2], "y: the samples of a row"),
                      (y.numpy(), r"y must be a \[n, rows, pitch\]")):
        with pytest.raises(ValueError, match=name):
            YuvFrames(bad, uv, 5, 7)
    with pytest.raises(ValueError, match="uv must be torch.uint8"):
        YuvFrames(y, uv.to(torch.int16), 5, 9)
    with pytest.raises(ValueError, match="y must be torch.uint16 or torch.int16"):
        YuvFrames(y, uv, 5, 9, fmt="p010")
    with pytest.raises(ValueError, match="YuvFrames"):
        yuv_to_rgb(torch.zeros(1, 3, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be"):
        yuv_to_rgb(s, out=torch.zeros(2, 3, 5, 10, dtype=torch.uint8))
    out = torch.full((2, 3, 5, 9), 7, dtype=torch.uint8)
    assert yuv_to_rgb(s, out=out) is out and torch.equal(out, yuv_to_rgb(s))


def test_from_surface_views_and_slicing():
    from mdqe_cvpr2023_amd.preprocess import YuvFrames, yuv_to_rgb
    n, H, W, pitch, crow = 5, 19, 37, 64, 32
    ys, cs = REF.make_content(3, n, H, W, "nv12")
    flat, rows = REF.pack(ys, cs, "nv12", pitch, crow, extra_rows=6)
    buf = torch.from_numpy(flat).view(n, rows, pitch)
    s = YuvFrames.from_surface(buf, H, W, crow, matrix="bt601", full_range=True, order="bgr")
    assert (len(s), s.height, s.width, s.matrix, s.full_range, s.order) == (n, H, W, "bt601", True, "bgr")
    assert s.y.data_ptr() == buf.data_ptr() and s.uv.data_ptr() == buf.data_ptr() + crow * pitch      # views: nothing is copied
    assert tuple(s.y.shape) == (n, H, pitch) and tuple(s.uv.shape) == (n, 10, pitch) and s.y.stride() == (rows * pitch, pitch, 1)
    want = REF.convert(ys, cs, H, W, "nv12", "bt601", True, "bgr")
    assert np.array_equal(yuv_to_rgb(s).numpy(), want)
    part = s[1:4]
    assert isinstance(part, YuvFrames) and len(part) == 3 and (part.height, part.width, part.matrix, part.full_range, part.order) == (H, W, "bt601", True, "bgr")
    assert part.y.data_ptr() == buf.data_ptr() + rows * pitch
    assert np.array_equal(yuv_to_rgb(part).numpy(), want[1:4])
    assert len(s[5:]) == 0 and tuple(yuv_to_rgb(s[5:]).shape) == (0, 3, H, W)
    assert np.array_equal(yuv_to_rgb(s[::2]).numpy(), want[::2])
    with pytest.raises(TypeError, match="slices"):
        s[0]
    used = s.used_rows()
    assert tuple(used.y.shape) == (n, H, pitch) and tuple(used.uv.shape) == (n, 10, pitch)
    moved = s.to("cpu")
    assert moved.y.is_contiguous() and moved.y.data_ptr() != s.y.data_ptr() and np.array_equal(yuv_to_rgb(moved).numpy(), want)
    for crow_bad, name in ((H - 1, "chroma_row"), (rows - 5, "buf holds")):
        with pytest.raises(ValueError, match=name):
            YuvFrames.from_surface(buf, H, W, crow_bad)
    with pytest.raises(ValueError, match="buf must be"):
        YuvFrames.from_surface(buf[0], H, W, crow)


def test_online_session_reads_the_size_of_surfaces():
    from mdqe_cvpr2023_amd.online import OnlineVideo
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    s = YuvFrames(torch.zeros(3, 6, 16, dtype=torch.uint8), torch.zeros(3, 3, 16, dtype=torch.uint8), 5, 9)
    assert OnlineVideo._hw(s) == (5, 9) and OnlineVideo._hw(torch.zeros(2, 3, 4, 7)) == (4, 7)


def test_the_image_branch_and_the_sharded_driver_refuse_surfaces():
    import dataclasses
    import types
    from mdqe_cvpr2023_amd import sharding
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    s = YuvFrames(torch.zeros(4, 8, 8, dtype=torch.uint8), torch.zeros(4, 4, 8, dtype=torch.uint8), 8, 8)
    # (a stand-in model as far as the driver looks at it before it would build its merger)
    cfg = PRESETS["R50_ovis_360"]
    geo = types.SimpleNamespace(Hp=8, Wp=8, N=4)
    model = types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"), engine=types.SimpleNamespace(geometry=lambda h, w: geo))
    with pytest.raises(ValueError, match="YuvFrames is not offered by the sharded driver"):
        sharding.run_round_robin(model, {0: s}, [(0, 0, 4)], 0, 1, None, (8, 8))
    with pytest.raises(ValueError, match="YuvFrames is not offered by the sharded driver"):
        sharding.run_round_robin(model, {}, [(0, 0, 4)], 0, 1, None, (8, 8), like=s)
    coco = types.SimpleNamespace(cfg=dataclasses.replace(cfg, is_coco=True), engine=None, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="YuvFrames: the COCO image branch"):
        MDQE.inference_image(coco, [{"image": s}])


def test_abi_declares_and_binds_the_entry_and_it_refuses_bad_arguments():
    from mdqe_cvpr2023_amd import _lib
    name = "mdqe_yuv420sp_to_rgb_u8"
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
    assert hasattr(h, name) and name in _lib.SIGNATURES
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == 15
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # no existing entry changed
    fn = getattr(h, name)

    def call(y=None, yp=64, ys=64 * 48, uv=None, cp=64, cs=64 * 48, NI=1, H=32, W=64, fmt=0, matrix=0, full=0, bgr=0, out=None):
        return fn(y, yp, ys, uv, cp, cs, NI, H, W, fmt, matrix, full, bgr, out, None)
    # refused before any pointer is looked at (NULL everywhere: nothing can be launched)
    EINVAL, ENULL = 1, 3
    for kw in ({"H": 0}, {"W": 0}, {"H": -1}, {"W": -4}, {"NI": -1}, {"fmt": 2}, {"fmt": -1}, {"matrix": 2},
               {"yp": 63}, {"cp": 63}, {"W": 63, "yp": 62}, {"W": 63, "yp": 63, "cp": 63},          # 63 pixels: 32 chroma pairs = 64 bytes
               {"fmt": 1, "yp": 127, "cp": 128}, {"fmt": 1, "yp": 128, "cp": 127},                 # P010: a row is 2 * W bytes
               {"fmt": 1, "yp": 129, "cp": 128}, {"fmt": 1, "yp": 128, "cp": 130, "ys": 128 * 48 + 1}, {"fmt": 1, "yp": 128, "cp": 128, "cs": 4097},
               {"ys": -64}, {"cs": -1},
               {"NI": 1 << 20, "H": 1024, "W": 1024, "yp": 1024, "cp": 1024},                      # NI * 3 * H * W >= 2^31
               {"NI": 1, "H": 30000, "W": 30000, "yp": 30000, "cp": 30000}):
        assert call(**kw) == EINVAL, kw
        assert call(**dict(kw, NI=kw.get("NI", 0))) == EINVAL, kw                                   # ... whatever NI says
    assert call(NI=0) == 0 and call(NI=0, fmt=1, yp=128, cp=128) == 0                               # NI = 0: OK, nothing launched
    assert call(W=63, yp=63, cp=64, NI=0) == 0                                                      # the tightest legal pitches
    assert call() == ENULL
    # odd P010 plane pointers (never dereferenced: the refusal comes before the launch)
    assert call(fmt=1, yp=128, cp=128, y=4097, uv=8192, out=4096) == EINVAL
    assert call(fmt=1, yp=128, cp=128, y=4096, uv=8193, out=4096) == EINVAL
