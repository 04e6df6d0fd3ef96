"""The conversion rule of mdqe_yuv420sp_to_rgb_u8 (include/mdqe_hip.h) restated in numpy int64: the oracle of the YUV input tests.
Integers only, so every comparison against it is exact.  Independent of the package's table: the constants are derived here from Kr, Kb.

Also the surface maker: random content plus the extremes of both ranges, packed into decoder-style allocations -- a row pitch wider
than the picture, the chroma plane at a chosen row offset, surfaces at a fixed distance, every byte of padding a poison byte, and (P010)
random low 6 bits in every word.
"""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
POISON = 0xAB


def gains(matrix, full_range, bits):
    """(yo, co, luma gain, (rv, gu, gv, bu)) of the float matrix for samples of `bits` bits: RGB = 0..255."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    top = (1 << bits) - 1
    sh = bits - 8
    if full_range:
        yo, gy, gc = 0, 255.0 / top, 255.0 / top
    else:
        yo, gy, gc = 16 << sh, 255.0 / (219 << sh), 255.0 / (224 << sh)
    return yo, 128 << sh, gy, tuple(g * gc for g in (2 * (1 - kr), -2 * kb * (1 - kb) / kg, -2 * kr * (1 - kr) / kg, 2 * (1 - kb)))


def coeffs(matrix, full_range, bits):
    """The integer constants (yo, co, cy, rv, gu, gv, bu): rint(gain * 65536)."""
    yo, co, gy, gc = gains(matrix, full_range, bits)
    return (yo, co, int(np.rint(gy * 65536))) + tuple(int(np.rint(g * 65536)) for g in gc)


def rule(Y, U, V, matrix, full_range, bits):
    """The integer rule on arrays of samples (any common shape) -> (R, G, B) int64 in 0..255, and the largest |accumulator|."""
    yo, co, cy, rv, gu, gv, bu = coeffs(matrix, full_range, bits)
    y = (np.asarray(Y, dtype=np.int64) - yo) * cy
    u, v = np.asarray(U, dtype=np.int64) - co, np.asarray(V, dtype=np.int64) - co
    acc = (y + rv * v + 32768, y + gu * u + gv * v + 32768, y + bu * u + 32768)
    return tuple(np.clip(a >> 16, 0, 255) for a in acc), max(int(np.abs(a).max()) for a in acc)


def float_rule(Y, U, V, matrix, full_range, bits):
    """clamp(rint(the float64 matrix)) -> (R, G, B) int64."""
    yo, co, gy, (rv, gu, gv, bu) = gains(matrix, full_range, bits)
    y = (np.asarray(Y, dtype=np.float64) - yo) * gy
    u, v = np.asarray(U, dtype=np.float64) - co, np.asarray(V, dtype=np.float64) - co
    return tuple(np.clip(np.rint(a), 0, 255).astype(np.int64) for a in (y + rv * v, y + gu * u + gv * v, y + bu * u))


def convert(ys, cs, H, W, fmt, matrix, full_range, order):
    """Samples -> uint8 [n, 3, H, W].  ys [n, H, W] luma samples, cs [n, ceil(H/2), 2*ceil(W/2)] interleaved chroma samples: bytes (NV12)
    or 16-bit words whose value is word >> 6 (P010)."""
    bits = 8 if fmt == "nv12" else 10
    ys, cs = np.asarray(ys).astype(np.int64), np.asarray(cs).astype(np.int64)
    if fmt == "p010":
        ys, cs = (ys & 0xFFFF) >> 6, (cs & 0xFFFF) >> 6
    r, c = np.arange(H)[:, None], np.arange(W)[None, :]
    U, V = cs[:, r >> 1, 2 * (c >> 1)], cs[:, r >> 1, 2 * (c >> 1) + 1]
    (R, G, B), _ = rule(ys, U, V, matrix, full_range, bits)
    planes = (R, G, B) if order == "rgb" else (B, G, R)
    return np.stack(planes, 1).astype(np.uint8)


EXTREMES = {"nv12": (0, 16, 235, 240, 255), "p010": (0, 64, 940, 960, 1023)}


def make_content(seed, n, H, W, fmt):
    """(ys [n, H, W], cs [n, ceil(H/2), 2*ceil(W/2)]) as the surface's own sample type (uint8; uint16 words with random low 6 bits):
    random values, every fourth sample or so one of the extremes of the two ranges."""
    rng = np.random.default_rng(seed)
    bits = 8 if fmt == "nv12" else 10
    ext = np.array(EXTREMES[fmt], dtype=np.int64)
    out = []
    for shape in ((n, H, W), (n, (H + 1) // 2, 2 * ((W + 1) // 2))):
        v = rng.integers(0, 1 << bits, size=shape)
        v = np.where(rng.random(shape) < 0.25, ext[rng.integers(0, len(ext), size=shape)], v)
        if fmt == "p010":
            v = (v << 6) | rng.integers(0, 64, size=shape)
        out.append(v.astype(np.uint8 if fmt == "nv12" else np.uint16))
    return out[0], out[1]


def tight_pitch(W, fmt):
    """Bytes of the longer of a luma row and a chroma row."""
    return 2 * ((W + 1) // 2) * (1 if fmt == "nv12" else 2)


def pack(ys, cs, fmt, pitch, chroma_row, extra_rows=0, lead=0):
    """The content as ONE allocation of bytes: `lead` poison bytes, then n surfaces of (chroma_row + chroma rows + extra_rows) rows of
    `pitch` bytes -- luma from row 0, chroma from row `chroma_row`, everything else poison.  -> (flat uint8 array, rows per surface)."""
    n, H, W = ys.shape
    ch = cs.shape[1]
    rows = chroma_row + ch + extra_rows
    assert chroma_row >= H and pitch >= tight_pitch(W, fmt)
    buf = np.full((n, rows, pitch), POISON, dtype=np.uint8)
    yb = ys.astype("<u2").view(np.uint8).reshape(n, H, -1) if fmt == "p010" else ys
    cb = cs.astype("<u2").view(np.uint8).reshape(n, ch, -1) if fmt == "p010" else cs
    buf[:, :H, :yb.shape[2]] = yb
    buf[:, chroma_row:chroma_row + ch, :cb.shape[2]] = cb
    return np.concatenate([np.full(lead, POISON, dtype=np.uint8), buf.reshape(-1)]), rows


def plane_views(flat, n, H, W, fmt, pitch, chroma_row, rows, lead=0, full_pitch=True):
    """The luma and chroma planes of a packed allocation (a flat torch uint8 tensor, host or device) as strided views, typed for the
    format: [n, H, pitch or W] and [n, ceil(H/2), pitch or 2*ceil(W/2)] in samples.  full_pitch=False: the last dimension stops at
    the picture (the views then cover no padding at all)."""
    import torch
    es = 1 if fmt == "nv12" else 2
    assert lead % es == 0 and pitch % es == 0
    t = flat if fmt == "nv12" else flat.view(torch.int16)
    p, ch, cw = pitch // es, (H + 1) // 2, 2 * ((W + 1) // 2)
    y = t.as_strided((n, H, p if full_pitch else W), (rows * p, p, 1), lead // es)
    uv = t.as_strided((n, ch, p if full_pitch else cw), (rows * p, p, 1), lead // es + chroma_row * p)
    return y, uv
