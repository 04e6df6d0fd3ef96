"""The painting rule of mdqe_render_overlay_yuv420sp (include/mdqe_hip.h) and the palette table of render.palette_yuv restated in numpy
int64: the oracle of the surface-overlay tests.  Written from the header's text, integers only, so every comparison against it is exact.
Independent of the package's table: the forward constants are derived here from Kr, Kb.

The round trip of the DEFAULT palette (render.default_palette(), rows as R, G, B) through `palette_yuv` and back through the existing
YUV -> RGB rule (tests/_yuv_ref.rule): the worst error of any channel of any of the 256 rows, per table row.  A deterministic integer
function, so tests/test_overlay_yuv_cpu.py asserts exactly these values (a pin, not a tolerance):

    nv12 bt601 limited 2    nv12 bt601 full 1    nv12 bt709 limited 2    nv12 bt709 full 1    (levels of 255; the 2 is in B)
    p010 (all four rows)  0                                                                      (ROUND_TRIP_WORST below)

Also the label-map maker: blobs that touch the row ends, the last (odd) row and column and the 16-pixel block borders, plus salt noise,
with labels from the whole range 0..255.
"""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}

# measured once (see the docstring); keys (fmt, matrix, full_range)
ROUND_TRIP_WORST = {
    ("nv12", "bt601", False): 2,
    ("nv12", "bt601", True): 1,
    ("nv12", "bt709", False): 2,
    ("nv12", "bt709", True): 1,
    ("p010", "bt601", False): 0,
    ("p010", "bt601", True): 0,
    ("p010", "bt709", False): 0,
    ("p010", "bt709", True): 0,
}


def forward_table(matrix, full_range, bits):
    """(yo, co, (ar, ag, ab), (ur, ug, ub), (vr, vg, vb)): rint(x * 65536) of the forward matrix for samples of `bits` bits from RGB
    0..255, the G entry of each row taking the rounding residue (luma row: sums to the rounded scale; chroma rows: sum to 0)."""
    kr, kb = KR_KB[matrix]
    sh, top = bits - 8, (1 << bits) - 1
    if full_range:
        yo, ys, cs = 0, top / 255.0, top / 255.0
    else:
        yo, ys, cs = 16 << sh, (219 << sh) / 255.0, (224 << sh) / 255.0

    def q(x):
        return int(np.rint(x * 65536))
    ar, ab = q(kr * ys), q(kb * ys)
    ur, ub = q(-kr / (2 * (1 - kb)) * cs), q(0.5 * cs)
    vr, vb = q(0.5 * cs), q(-kb / (2 * (1 - kr)) * cs)
    return yo, 128 << sh, (ar, q(ys) - ar - ab, ab), (ur, -(ur + ub), ub), (vr, -(vr + vb), vb)


def palette_yuv(palette_rgb, fmt, matrix, full_range, order="rgb"):
    """uint8 [256, 3] (rows in channel order `order`) -> int64 [256, 3] rows (Y, U, V) in sample units."""
    bits = 8 if fmt == "nv12" else 10
    yo, co, ky, ku, kv = forward_table(matrix, full_range, bits)
    p = np.asarray(palette_rgb).astype(np.int64)
    assert p.shape == (256, 3)
    r, g, b = (p[:, 0], p[:, 1], p[:, 2]) if order == "rgb" else (p[:, 2], p[:, 1], p[:, 0])
    top = (1 << bits) - 1
    y = yo + ((ky[0] * r + ky[1] * g + ky[2] * b + 32768) >> 16)
    u = np.clip(co + ((ku[0] * r + ku[1] * g + ku[2] * b + 32768) >> 16), 0, top)        # (>> on int64: arithmetic, floor)
    v = np.clip(co + ((kv[0] * r + kv[1] * g + kv[2] * b + 32768) >> 16), 0, top)
    return np.stack([y, u, v], 1)


def edges(lab, contour):
    """bool [F, H, W]: for some d in 1..contour the neighbour at (+-d, 0) or (0, +-d) lies inside the picture and has another label."""
    F, H, W = lab.shape
    e = np.zeros(lab.shape, dtype=bool)
    for d in range(1, contour + 1):
        for dr, dc in ((-d, 0), (d, 0), (0, -d), (0, d)):
            r0, r1 = max(0, -dr), min(H, H - dr)                      # the pixels whose neighbour (r + dr, c + dc) is inside
            c0, c1 = max(0, -dc), min(W, W - dc)
            if r0 < r1 and c0 < c1:
                e[:, r0:r1, c0:c1] |= lab[:, r0:r1, c0:c1] != lab[:, r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return e


def paint(ys, cs, labels, pal_yuv, fmt, a256=128, contour=1):
    """Stored samples in, stored samples out: ys [F, H, W], cs [F, ceil(H/2), 2*ceil(W/2)] (bytes for "nv12"; 16-bit words whose value
    is word >> 6 for "p010"), labels uint8 [F, H, W], pal_yuv [256, 3] -> (ys', cs') of the same dtypes."""
    p010 = fmt == "p010"
    lab = np.asarray(labels)
    F, H, W = lab.shape
    assert lab.dtype == np.uint8 and 0 <= a256 <= 256 and 0 <= contour <= 3
    ry, rc = np.asarray(ys).astype(np.int64) & 0xFFFF, np.asarray(cs).astype(np.int64) & 0xFFFF
    assert ry.shape == (F, H, W) and rc.shape == (F, (H + 1) // 2, 2 * ((W + 1) // 2))
    pal = np.asarray(pal_yuv).astype(np.int64)
    l = lab.astype(np.int64)
    edge = edges(lab, contour)

    def px(s, p):
        return np.where(l == 0, s, np.where(edge, p, (s * (256 - a256) + p * a256 + 128) >> 8))
    Y = ry >> 6 if p010 else ry
    yout = px(Y, pal[l, 0])
    oy = np.where(l == 0, ry, yout << 6 if p010 else yout)
    oc = rc.copy()
    for br in range((H + 1) // 2):
        for bc in range((W + 1) // 2):
            rows, cols = [r for r in (2 * br, 2 * br + 1) if r < H], [c for c in (2 * bc, 2 * bc + 1) if c < W]
            n = len(rows) * len(cols)                                 # 1, 2 or 4
            sh = {1: 0, 2: 1, 4: 2}[n]
            labelled = np.zeros(F, dtype=bool)
            for r in rows:
                for c in cols:
                    labelled |= l[:, r, c] != 0
            for k in (0, 1):                                          # U, V
                raw = rc[:, br, 2 * bc + k]
                C = raw >> 6 if p010 else raw
                total = np.zeros(F, dtype=np.int64)
                for r in rows:
                    for c in cols:
                        lv, ev = l[:, r, c], edge[:, r, c]
                        p = pal[lv, 1 + k]
                        total += np.where(lv == 0, C, np.where(ev, p, (C * (256 - a256) + p * a256 + 128) >> 8))
                cout = (total + n // 2) >> sh
                oc[:, br, 2 * bc + k] = np.where(labelled, cout << 6 if p010 else cout, raw)
    dt = np.uint16 if p010 else np.uint8
    return oy.astype(dt), oc.astype(dt)


def make_labels(seed, F, H, W):
    """uint8 [F, H, W]: background, rectangular and round blobs with labels from 1..255 -- some pinned to the first / last column, the
    last row and the columns around every multiple of 16 -- and 3 % salt noise of any label 0..255."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((F, H, W), dtype=np.uint8)
    rr, cc = np.arange(H)[:, None], np.arange(W)[None, :]
    for f in range(F):
        anchors = [(0, 0), (H - 1, W - 1), (H - 1, 0), (0, W - 1)] + [(int(rng.integers(0, H)), c) for c in range(16, W, 16)]
        anchors += [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(3)]
        for i, (r, c) in enumerate(anchors):
            if i and rng.random() < 0.3:
                continue
            label = int(rng.integers(1, 256)) if i != 1 else 255
            hr, hc = int(rng.integers(1, max(2, H // 2 + 1))), int(rng.integers(1, max(2, W // 3 + 1)))
            if rng.random() < 0.5:
                m = (np.abs(rr - r) < hr) & (np.abs(cc - c) < hc)
            else:
                m = ((rr - r) * hc) ** 2 + ((cc - c) * hr) ** 2 < (hr * hc) ** 2
            lab[f][m] = label
        salt = rng.random((H, W)) < 0.03
        lab[f][salt] = rng.integers(0, 256, size=int(salt.sum()))
    return lab
