"""Eval-time input side on the device.

The reference's YTVISDatasetMapper resizes every decoded frame on the host before the model sees it
(mdqe/data/dataset_mapper.py:252-258: ResizeShortestEdgeClip -> detectron2 ResizeTransform -> PIL
`Image.resize(BILINEAR)` for uint8 images; size rule mdqe/data/augmentation.py:376-389).  Here the decoded frames go to
the GPU at their native size and are resized there, bit-identical to Pillow: the same separable fixed-point resampling
(csrc/spatial.hip: resize_pil_bilinear_kernel), with the coefficient tables Pillow would build computed on the host in
double precision.  Normalisation and zero padding stay fused into the stem's im2col kernel.
"""
import numpy as np
import torch

from ._lib import check, cur_stream, lib, ptr

PRECISION_BITS = 32 - 8 - 2
_tables = {}


def shortest_edge_size(h, w, size, max_size):
    """ResizeShortestEdgeClip.get_transform (mdqe/data/augmentation.py:376-389): output (h, w)."""
    scale = size * 1.0 / min(h, w)
    if h < w:
        newh, neww = size, scale * w
    else:
        newh, neww = scale * h, size
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def pil_bilinear_coeffs(in_size, out_size):
    """Pillow precompute_coeffs + normalize_coeffs_8bpc (Resample.c), bilinear filter, whole axis; vectorised.
    -> xmin int32 [out], cnt int32 [out], k int32 [out, ksize]."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx + 0.5) * scale
    x0 = np.maximum((center - support + 0.5).astype(np.int64), 0)
    x1 = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = x1 - x0
    t = np.arange(ksize, dtype=np.float64)[None]
    arg = np.abs((t + x0[:, None] - center[:, None] + 0.5) / filterscale)
    w = np.where((arg < 1.0) & (t < n[:, None]), 1.0 - arg, 0.0)
    ww = w.sum(1, keepdims=True)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    q = (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)           # weights are >= 0 for the triangle filter
    return x0.astype(np.int32), n.astype(np.int32), q.astype(np.int32)


def _dev_tables(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    if key not in _tables:
        while len(_tables) >= 64:                        # a few KB each; bounded all the same (oldest first)
            _tables.pop(next(iter(_tables)))
        x0, n, k = pil_bilinear_coeffs(in_size, out_size)
        _tables[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (x0, n, k)) + (int(k.shape[1]),)
    return _tables[key]


def resize_frames(frames, out_h, out_w):
    """frames: CUDA uint8 [NI, C, H, W] (contiguous) -> [NI, C, out_h, out_w] uint8, == PIL Image.resize(BILINEAR) per frame."""
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.is_contiguous()):
        raise RuntimeError("resize_frames: expected a contiguous CUDA uint8 [NI,C,H,W] tensor")
    NI, C, H, W = frames.shape
    if (H, W) == (out_h, out_w):
        return frames
    xm, xc, xk, kxs = _dev_tables(W, out_w, frames.device)
    ym, yc, yk, kys = _dev_tables(H, out_h, frames.device)
    out = torch.empty(NI, C, out_h, out_w, dtype=torch.uint8, device=frames.device)
    check(lib.mdqe_resize_pil_bilinear_u8(ptr(frames), C * H * W, NI, C, H, W, out_h, out_w, ptr(xm), ptr(xc), ptr(xk), kxs,
                                          ptr(ym), ptr(yc), ptr(yk), kys, ptr(out), cur_stream()), "resize_pil_bilinear")
    return out


def resize_shortest_edge(frames, min_size, max_size):
    """The eval augmentation of the reference on device-resident frames: [NI,C,H,W] uint8 -> resized uint8 frames."""
    oh, ow = shortest_edge_size(int(frames.shape[-2]), int(frames.shape[-1]), min_size, max_size)
    return resize_frames(frames, oh, ow)


# ---- decoder surfaces as video input: semi-planar YUV 4:2:0 (NV12, P010) -> planar uint8 RGB -----------------------------------------
# The rule is written once, in include/mdqe_hip.h (mdqe_yuv420sp_to_rgb_u8): integers only, chroma replicated.  This is its table of
# constants (the header's MDQE_YUV_COEFFS): (fmt, matrix, full_range) -> (yo, co, cy, rv, gu, gv, bu).
YUV_FORMATS = ("nv12", "p010")
YUV_MATRICES = ("bt601", "bt709")
YUV_COEFFS = {
    ("nv12", "bt601", False): (16, 128, 76309, 104597, -25675, -53279, 132201),
    ("nv12", "bt601", True): (0, 128, 65536, 91881, -22553, -46802, 116130),
    ("nv12", "bt709", False): (16, 128, 76309, 117489, -13975, -34925, 138438),
    ("nv12", "bt709", True): (0, 128, 65536, 103206, -12276, -30679, 121609),
    ("p010", "bt601", False): (64, 512, 19077, 26149, -6419, -13320, 33050),
    ("p010", "bt601", True): (0, 512, 16336, 22903, -5622, -11666, 28947),
    ("p010", "bt709", False): (64, 512, 19077, 29372, -3494, -8731, 34610),
    ("p010", "bt709", True): (0, 512, 16336, 25726, -3060, -7647, 30313),
}


class YuvFrames:
    """Frames of a video as decoder surfaces: a luma plane `y` [n, rows >= height, pitch >= width] and a chroma plane `uv` [n, rows >=
    ceil(height/2), pitch_uv >= 2*ceil(width/2)] of interleaved U, V samples; uint8 for fmt "nv12", torch.uint16 or torch.int16 (the
    same bits: 10-bit values in the top of little-endian 16-bit words) for "p010".  The last dimension has stride 1; the other strides
    are the row pitch and the distance between surfaces, whatever they are -- views into a decoder's allocation are not copied.  Host
    or device.  matrix "bt601" / "bt709", full_range, and order "rgb" / "bgr" (the plane order of the converted frames) choose the
    conversion; `yuv_to_rgb` performs it.  A YuvFrames goes wherever a video's frames go: {"image": YuvFrames(...)}, ov.push(...)."""

    def __init__(self, y, uv, height, width, fmt="nv12", matrix="bt709", full_range=False, order="rgb"):
        if fmt not in YUV_FORMATS:
            raise ValueError("YuvFrames: fmt must be one of %s, got %r" % (YUV_FORMATS, fmt))
        if matrix not in YUV_MATRICES:
            raise ValueError("YuvFrames: matrix must be one of %s, got %r" % (YUV_MATRICES, matrix))
        if order not in ("rgb", "bgr"):
            raise ValueError("YuvFrames: order must be 'rgb' or 'bgr', got %r" % (order,))
        if not isinstance(full_range, (bool, np.bool_)):
            raise ValueError("YuvFrames: full_range must be a bool, got %r" % (full_range,))
        for name, v in (("height", height), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("YuvFrames: %s must be an int >= 1, got %r" % (name, v))
        height, width = int(height), int(width)
        want = (torch.uint8,) if fmt == "nv12" else (torch.uint16, torch.int16)
        for name, t in (("y", y), ("uv", uv)):
            if not torch.is_tensor(t) or t.dim() != 3:
                raise ValueError("YuvFrames: %s must be a [n, rows, pitch] tensor" % name)
            if t.dtype not in want:
                raise ValueError("YuvFrames: %s must be %s for fmt %r, got %s" % (name, " or ".join(str(d) for d in want), fmt, t.dtype))
            if t.shape[2] > 1 and t.stride(2) != 1:
                raise ValueError("YuvFrames: %s: the samples of a row must be consecutive (stride 1 in the last dimension)" % name)
        if y.shape[1] < height or y.shape[2] < width:
            raise ValueError("YuvFrames: y holds %d rows of %d samples, the picture needs %d x %d" % (y.shape[1], y.shape[2], height, width))
        ch, cw = (height + 1) // 2, 2 * ((width + 1) // 2)
        if uv.shape[1] < ch or uv.shape[2] < cw:
            raise ValueError("YuvFrames: uv holds %d rows of %d samples, the picture needs %d x %d" % (uv.shape[1], uv.shape[2], ch, cw))
        if uv.shape[0] != y.shape[0]:
            raise ValueError("YuvFrames: uv holds %d surfaces, y %d" % (uv.shape[0], y.shape[0]))
        if uv.device != y.device:
            raise ValueError("YuvFrames: uv is on %s, y on %s" % (uv.device, y.device))
        if fmt == "p010":                                   # one dtype inside (uint16 has few ops of its own); the same bits
            y, uv = y.view(torch.int16), uv.view(torch.int16)
        self.y, self.uv, self.height, self.width = y, uv, height, width
        self.fmt, self.matrix, self.full_range, self.order = fmt, matrix, bool(full_range), order

    @classmethod
    def from_surface(cls, buf, height, width, chroma_row, **kw):
        """The two views of ONE decoder allocation: buf [n, rows, pitch], luma in rows 0 .. height-1, chroma from row `chroma_row` (the
        decoder's aligned height) on, both with the surface's pitch."""
        if not torch.is_tensor(buf) or buf.dim() != 3:
            raise ValueError("YuvFrames.from_surface: buf must be a [n, rows, pitch] tensor")
        if isinstance(chroma_row, bool) or not isinstance(chroma_row, (int, np.integer)) or chroma_row < int(height):
            raise ValueError("YuvFrames.from_surface: chroma_row must be an int >= height, got %r" % (chroma_row,))
        ch = (int(height) + 1) // 2
        if buf.shape[1] < chroma_row + ch:
            raise ValueError("YuvFrames.from_surface: buf holds %d rows, chroma_row %d + %d chroma rows need %d"
                             % (buf.shape[1], chroma_row, ch, chroma_row + ch))
        return cls(buf[:, :int(height)], buf[:, int(chroma_row):int(chroma_row) + ch], height, width, **kw)

    @classmethod
    def empty(cls, n, height, width, fmt="nv12", device="cpu", pitch_align=1, pin_memory=False, **kw):
        """n fresh surfaces, each plane an allocation of its own: luma [n, height, pitch], chroma [n, ceil(height/2), pitch_uv], the
        pitches tight (width and 2*ceil(width/2) samples) or, with pitch_align=k, rounded up to a multiple of k BYTES.  The samples
        are uninitialised; where a pitch leaves padding the plane is zero-filled.  (k = 1: tight for either format.)"""
        if fmt not in YUV_FORMATS:
            raise ValueError("YuvFrames: fmt must be one of %s, got %r" % (YUV_FORMATS, fmt))
        es = 1 if fmt == "nv12" else 2
        k = pitch_align
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or (k > 1 and k % es):
            raise ValueError("YuvFrames: pitch_align must be an int >= 1 in bytes%s, got %r" % (", even for p010" if es == 2 else "", k))
        planes = []
        for rows, samples in ((int(height), int(width)), ((int(height) + 1) // 2, 2 * ((int(width) + 1) // 2))):
            pitch = (samples * es + k - 1) // k * k // es
            make = torch.zeros if pitch > samples else torch.empty
            planes.append(make((int(n), rows, pitch), dtype=torch.uint8 if es == 1 else torch.int16, device=device,
                               pin_memory=bool(pin_memory)))
        return cls(planes[0], planes[1], height, width, fmt=fmt, **kw)

    @classmethod
    def cat(cls, parts):
        """Surfaces of one kind (size, fmt, matrix, range, order) in a row -> one YuvFrames (the planes are concatenated: a copy)."""
        parts = list(parts)
        if not parts or any(not isinstance(p, YuvFrames) or p.meta() != parts[0].meta() for p in parts):
            raise ValueError("YuvFrames.cat: expected one or more YuvFrames of the same size, fmt, matrix, range and order")
        return parts[0]._like(torch.cat([p.y for p in parts]), torch.cat([p.uv for p in parts]))

    def meta(self):
        """What the planes do not say: (height, width, fmt, matrix, full_range, order)."""
        return (self.height, self.width, self.fmt, self.matrix, self.full_range, self.order)

    def __len__(self):
        return int(self.y.shape[0])

    @property
    def device(self):
        return self.y.device

    @property
    def is_cuda(self):
        return self.y.is_cuda

    def clone(self):
        return self._like(self.y.clone(), self.uv.clone())

    def record_stream(self, stream):
        self.y.record_stream(stream)
        self.uv.record_stream(stream)

    def __getitem__(self, s):
        if not isinstance(s, slice):
            raise TypeError("YuvFrames: frames are taken by slices (surfaces[a:b])")
        return self._like(self.y[s], self.uv[s])

    def _like(self, y, uv):
        return YuvFrames(y, uv, self.height, self.width, fmt=self.fmt, matrix=self.matrix, full_range=self.full_range, order=self.order)

    def used_rows(self):
        """The rows the picture uses, nothing else: what an upload has to move."""
        return self._like(self.y[:, :self.height], self.uv[:, :(self.height + 1) // 2])

    def to(self, device, non_blocking=False):
        """The used rows of both planes on `device`, pitch kept (a fresh tensor per plane; the caller orders the copy)."""
        u = self.used_rows()
        out = []
        for t in (u.y, u.uv):
            d = torch.empty(tuple(t.shape), dtype=t.dtype, device=device)
            d.copy_(t, non_blocking=non_blocking)
            out.append(d)
        return self._like(*out)


def _pitch_stride(t):
    """(row pitch, surface stride) of a plane in bytes; a dimension of size 1 has no stride of its own."""
    es = t.element_size()
    pitch = t.stride(1) if t.shape[1] > 1 else t.shape[2]
    stride = t.stride(0) if t.shape[0] > 1 else t.shape[1] * pitch
    return pitch * es, stride * es


def yuv_to_rgb(yuv, out=None):
    """YuvFrames -> uint8 [n, 3, height, width], contiguous, planes in `yuv.order`, on the device the planes are on (`out`: such a
    tensor to write into, e.g. rows of a larger store).  On a HIP device one launch of mdqe_yuv420sp_to_rgb_u8 on the current stream;
    on the CPU the same rule in torch int32."""
    if not isinstance(yuv, YuvFrames):
        raise ValueError("yuv_to_rgb: expected a YuvFrames, got %s" % type(yuv).__name__)
    n, H, W = len(yuv), yuv.height, yuv.width
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.uint8, device=yuv.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and tuple(out.shape) == (n, 3, H, W) and out.is_contiguous()
              and out.device == yuv.device):
        raise ValueError("yuv_to_rgb: out must be a contiguous uint8 [%d, 3, %d, %d] tensor on %s" % (n, H, W, yuv.device))
    if yuv.y.is_cuda:
        yp, ys = _pitch_stride(yuv.y)
        cp, cs = _pitch_stride(yuv.uv)
        with torch.cuda.device(yuv.device):
            check(lib.mdqe_yuv420sp_to_rgb_u8(ptr(yuv.y), yp, ys, ptr(yuv.uv), cp, cs, n, H, W, YUV_FORMATS.index(yuv.fmt),
                                              YUV_MATRICES.index(yuv.matrix), int(yuv.full_range), int(yuv.order == "bgr"), ptr(out),
                                              cur_stream(yuv.device)), "yuv420sp_to_rgb")
        return out
    yo, co, cy, rv, gu, gv, bu = YUV_COEFFS[(yuv.fmt, yuv.matrix, yuv.full_range)]
    ch, cw = (H + 1) // 2, (W + 1) // 2

    def samples(t):
        v = t.to(torch.int32)
        return v if yuv.fmt == "nv12" else (v & 0xFFFF) >> 6
    y = (samples(yuv.y[:, :H, :W]) - yo) * cy
    c = samples(yuv.uv[:, :ch, :2 * cw]).reshape(n, ch, cw, 2) - co
    c = c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W]          # chroma replicated: [r >> 1][c >> 1]
    u, v = c[..., 0], c[..., 1]
    planes = [y + rv * v, y + gu * u + gv * v, y + bu * u]
    if yuv.order == "bgr":
        planes.reverse()
    for k, p in enumerate(planes):
        out[:, k] = ((p + 32768) >> 16).clamp_(0, 255).to(torch.uint8)
    return out
