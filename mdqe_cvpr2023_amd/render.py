"""How an overlay is painted (model.overlay_output, online_video(emit="overlay")): the palette and the style.  The painting itself is
ops.render_overlay (csrc/render.hip) behind the label map; merge.overlay_frames puts the two together for a tracker window.  A style
with a mosaic (redaction) is painted by ops.render_mosaic (csrc/render_mosaic.hip) from the style's per-label action table, one with a
blur by ops.render_blur (csrc/render_blur.hip) from the same table and the tap tables of `blur_taps`.  A style with a margin
(`grow`) has ops.grow_labels (csrc/grow.hip) dilate the labels of its `grows` table first, and the painter takes that map.  A style
with a box or a caption has ops.annotate (csrc/annotate.hip) draw them onto the painted picture, from the label map's geometry table,
the font, the ink colours and the window's caption table made here.  `Crops` is the request for the other picture made from the same
trio of frames, label map and geometry table: one fixed-size chip per track and frame (ops.track_crops, csrc/crops.hip).

A track's colour depends only on its tracker row (label = row + 1), so it keeps its colour across windows and pushes."""
import dataclasses
import math

import torch

_HUE_STEPS = 1536                 # 6 sectors of 256 integer steps
_HUE_STRIDE = 949                 # round(1536 / golden ratio); odd and no multiple of 3: coprime with 1536, every label its own hue
_BANDS = ((255, 0), (255, 112), (176, 0))      # (largest, smallest channel) by (label - 1) % 3: vivid, pastel, dark


def _label_colour(label):
    """Integers only: the hue walks the circle in golden-ratio steps (neighbouring labels land far apart, and so do labels 2, 3, ... apart),
    the band changes saturation / value with every label."""
    if label == 0:
        return (0, 0, 0)
    hue = (label * _HUE_STRIDE) % _HUE_STEPS
    hi, lo = _BANDS[(label - 1) % 3]
    sector, t = divmod(hue, 256)
    up = lo + ((hi - lo) * t + 127) // 255
    down = hi - ((hi - lo) * t + 127) // 255
    return ((hi, up, lo), (down, hi, lo), (lo, hi, up), (lo, down, hi), (up, lo, hi), (hi, lo, down))[sector]


def default_palette():
    """uint8 [256, 3] on the host, a pure integer function of the label (no float hue maths whose rounding could differ between hosts).
    Row 0 is black; rows 1..255 are pairwise distinct, any two labels fewer than 8 apart differ by at least 64 in L1, and every row's
    largest channel is at least 128 (visible on black).  Channel order: whatever the frames' is -- the rows are (first, second, third)
    channel of the frames handed in."""
    return torch.tensor([_label_colour(i) for i in range(256)], dtype=torch.uint8)


# RGB (0..255) -> YUV samples, the table of `palette_yuv`: (fmt, matrix, full_range) -> (yo, co, (ar, ag, ab), (ur, ug, ub), (vr, vg, vb)).
# rint(x * 65536) of the standard forward matrices, the inverses of the header's MDQE_YUV_COEFFS: luma row (Kr, Kg, Kb) times 219/255,
# 876/255, 1 or 1023/255; chroma rows (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)) and (1 - Kr, -Kg, -Kb) / (2 (1 - Kr)) times 224/255, 896/255, 1
# or 1023/255.  The G entry takes the rounding residue: a luma row sums to the rounded scale, a chroma row to 0, so a grey has exactly
# neutral chroma and black / white land on the nominal codes.
YUV_FORWARD = {
    ("nv12", "bt601", False): (16, 128, (16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681)),
    ("nv12", "bt601", True): (0, 128, (19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329)),
    ("nv12", "bt709", False): (16, 128, (11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639)),
    ("nv12", "bt709", True): (0, 128, (13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005)),
    ("p010", "bt601", False): (64, 512, (67315, 132155, 25665), (-38856, -76282, 115138), (115138, -96414, -18724)),
    ("p010", "bt601", True): (0, 512, (78612, 154331, 29972), (-44363, -87095, 131458), (131458, -110080, -21378)),
    ("p010", "bt709", False): (64, 512, (47864, 161016, 16255), (-26383, -88755, 115138), (115138, -104581, -10557)),
    ("p010", "bt709", True): (0, 512, (55896, 188037, 18982), (-30123, -101335, 131458), (131458, -119404, -12054)),
}


def palette_yuv(palette_rgb, fmt="nv12", matrix="bt709", full_range=False, order="rgb"):
    """An overlay palette (uint8 [256, 3], rows in the frames' channel order `order`: "rgb" or "bgr") in the samples of a decoder
    surface: uint16 [256, 3] on the host, rows (Y, U, V), 0..255 for "nv12" and 0..1023 for "p010" -- what ops.render_overlay_yuv
    paints with.  Integers only: Y = yo + ((ar*R + ag*G + ab*B + 32768) >> 16); U, V = co + ((.. + 32768) >> 16) with the arithmetic
    shift (floor), clamped to the sample range (YUV_FORWARD)."""
    if not torch.is_tensor(palette_rgb) or palette_rgb.dtype != torch.uint8 or tuple(palette_rgb.shape) != (256, 3):
        raise ValueError("palette_yuv: palette_rgb must be a uint8 [256, 3] tensor")
    if (fmt, matrix, full_range) not in YUV_FORWARD or not isinstance(full_range, bool) or order not in ("rgb", "bgr"):
        raise ValueError("palette_yuv: fmt 'nv12' / 'p010', matrix 'bt601' / 'bt709', full_range a bool, order 'rgb' / 'bgr'; got %r"
                         % ((fmt, matrix, full_range, order),))
    yo, co, ky, ku, kv = YUV_FORWARD[(fmt, matrix, full_range)]
    top = 255 if fmt == "nv12" else 1023
    p = palette_rgb.cpu().to(torch.int64)
    r, g, b = (p[:, 0], p[:, 1], p[:, 2]) if order == "rgb" else (p[:, 2], p[:, 1], p[:, 0])
    rows = [yo + ((ky[0] * r + ky[1] * g + ky[2] * b + 32768) >> 16)]
    rows += [(co + ((k[0] * r + k[1] * g + k[2] * b + 32768) >> 16)).clamp(0, top) for k in (ku, kv)]
    return torch.stack(rows, 1).to(torch.uint16)


def backdrop_yuv(colour, fmt="nv12", matrix="bt709", full_range=False, order="rgb"):
    """A backdrop colour (three ints 0..255 in the frames' channel order `order`) in the samples of a decoder surface: uint16 [3] on the
    host, (Y, U, V) -- what ops.render_replace_yuv mixes with.  `palette_yuv`'s integers: a grey has exactly neutral chroma."""
    c = _backdrop(colour, "backdrop_yuv")
    if torch.is_tensor(c):
        raise ValueError("backdrop_yuv: colour must be three ints 0..255, got a tensor (a picture backdrop of a surface session is a "
                         "YuvFrames of one surface)")
    if not isinstance(c, tuple):
        raise ValueError("backdrop_yuv: colour must be three ints 0..255, got %r" % (colour,))
    pal = torch.zeros(256, 3, dtype=torch.uint8)
    pal[0] = torch.tensor(c, dtype=torch.uint8)
    return palette_yuv(pal, fmt, matrix, full_range, order)[0].contiguous()


# The annotation pass's font (ops.annotate, csrc/annotate.hip): 5 x 7 glyphs for 0x20..0x5F drawn for this project, one per line, 7 rows
# top to bottom as hex, bit 4 the leftmost pixel of a row.
_FONT = """
  00 00 00 00 00 00 00
! 04 04 04 04 04 00 04
" 0A 0A 0A 00 00 00 00
# 0A 0A 1F 0A 1F 0A 0A
$ 04 0F 14 0E 05 1E 04
% 18 19 02 04 08 13 03
& 0C 12 14 08 15 12 0D
' 0C 04 08 00 00 00 00
( 02 04 08 08 08 04 02
) 08 04 02 02 02 04 08
* 00 04 15 0E 15 04 00
+ 00 04 04 1F 04 04 00
, 00 00 00 00 0C 04 08
- 00 00 00 1F 00 00 00
. 00 00 00 00 00 0C 0C
/ 00 01 02 04 08 10 00
0 0E 11 13 15 19 11 0E
1 04 0C 04 04 04 04 0E
2 0E 11 01 02 04 08 1F
3 1F 02 04 02 01 11 0E
4 02 06 0A 12 1F 02 02
5 1F 10 1E 01 01 11 0E
6 06 08 10 1E 11 11 0E
7 1F 01 02 04 08 08 08
8 0E 11 11 0E 11 11 0E
9 0E 11 11 0F 01 02 0C
: 00 0C 0C 00 0C 0C 00
; 00 0C 0C 00 0C 04 08
< 02 04 08 10 08 04 02
= 00 00 1F 00 1F 00 00
> 08 04 02 01 02 04 08
? 0E 11 01 02 04 00 04
@ 0E 11 01 0D 15 15 0E
A 0E 11 11 11 1F 11 11
B 1E 11 11 1E 11 11 1E
C 0E 11 10 10 10 11 0E
D 1C 12 11 11 11 12 1C
E 1F 10 10 1E 10 10 1F
F 1F 10 10 1E 10 10 10
G 0E 11 10 17 11 11 0F
H 11 11 11 1F 11 11 11
I 0E 04 04 04 04 04 0E
J 07 02 02 02 02 12 0C
K 11 12 14 18 14 12 11
L 10 10 10 10 10 10 1F
M 11 1B 15 15 11 11 11
N 11 11 19 15 13 11 11
O 0E 11 11 11 11 11 0E
P 1E 11 11 1E 10 10 10
Q 0E 11 11 11 15 12 0D
R 1E 11 11 1E 14 12 11
S 0F 10 10 0E 01 01 1E
T 1F 04 04 04 04 04 04
U 11 11 11 11 11 11 0E
V 11 11 11 11 11 0A 04
W 11 11 11 15 15 15 0A
X 11 11 0A 04 0A 11 11
Y 11 11 11 0A 04 04 04
Z 1F 01 02 04 08 10 1F
[ 0E 08 08 08 08 08 0E
\\ 00 10 08 04 02 01 00
] 0E 02 02 02 02 02 0E
^ 04 0A 11 00 00 00 00
_ 00 00 00 00 00 00 1F
"""

CAP_LEN = 32                      # bytes of a caption row: longer texts are cut
CAPTIONS = (None, "id", "class", "id+class", "id+class+score", "class+score")


def default_font():
    """uint8 [64, 7] on the host: glyph ch - 32 for ch in 0x20..0x5F (row 0 is the space), 7 rows top to bottom, bit 4 - x of a row is
    its pixel x = 0..4 -- the layout ops.annotate reads."""
    lines = _FONT.strip("\n").split("\n")
    assert len(lines) == 64 and all(ord(line[0]) == 32 + i for i, line in enumerate(lines))
    return torch.tensor([[int(v, 16) for v in line[2:].split()] for line in lines], dtype=torch.uint8)


def ink(palette):
    """The colour of the text on each label's plate, uint8 [256, 3] on the host: row l is white where palette row l is dark
    (c0 + c1 + c2 < 384), else black.  For surfaces: palette_yuv(ink(palette), ...) -- black and white do not depend on the channel order."""
    if not torch.is_tensor(palette) or palette.dtype != torch.uint8 or tuple(palette.shape) != (256, 3):
        raise ValueError("ink: palette must be a uint8 [256, 3] tensor")
    dark = palette.cpu().to(torch.int64).sum(1) < 384
    return torch.where(dark[:, None], 255, 0).to(torch.uint8).expand(256, 3).contiguous()


def captions(style, cls_probs, n):
    """The caption table of ops.annotate, uint8 [256, CAP_LEN] on the host, a pure function: row l is the text of label l = tracker row
    l - 1 for l in 1..n, the fields `style.caption` lists joined by single spaces -- id: the tracker row in decimal; class:
    style.class_names[j] upper-cased (without names: j in decimal) for j the first maximum of row l - 1 of the window's class rows
    cls_probs [>= n, K]; score: int(100 * p + 0.5) of that maximum p (the float32 value as a Python float) and '%' -- cut to CAP_LEN
    bytes and ended by 0 bytes.  Row 0 and the rows above n are empty."""
    table = torch.zeros(256, CAP_LEN, dtype=torch.uint8)
    fields = style.caption.split("+") if style.caption else []
    n = min(int(n), 255)
    if not fields or n <= 0:
        return table
    first = top = None
    if fields != ["id"]:
        if not torch.is_tensor(cls_probs) or cls_probs.dim() != 2 or cls_probs.shape[0] < n or cls_probs.shape[1] < 1:
            raise ValueError("overlay style: caption %r needs the window's class rows [>= %d, K >= 1], got %s"
                             % (style.caption, n, tuple(cls_probs.shape) if torch.is_tensor(cls_probs) else type(cls_probs).__name__))
        rows = cls_probs[:n].detach().cpu().float()
        first = rows.argmax(1).tolist()                 # (of several maxima the first: torch.argmax's rule)
        top = rows.max(1)[0].tolist()
    names = style.class_names
    for t in range(n):
        parts = []
        for field in fields:
            if field == "id":
                parts.append(str(t))
            elif field == "class":
                j = first[t]
                parts.append(str(names[j]).upper() if names is not None and j < len(names) else str(j))
            else:
                parts.append("%d%%" % int(100 * top[t] + 0.5))
        text = " ".join(parts).encode("ascii", "replace")[:CAP_LEN]
        table[t + 1, :len(text)] = torch.tensor(list(text), dtype=torch.uint8)
    return table


def blur_taps(radius):
    """The taps of the blur painters (ops.render_blur, csrc/render_blur.hip), uint16 [radius + 1] on the host, a pure function: a
    Gaussian of sigma = radius / 2 cut at `radius`, g[d] = exp(-2 d^2 / radius^2), in units of 1/4096 -- w[d] = rint(4096 g[d] / G) for
    d >= 1 with G = g[0] + 2 sum(g[1:]), and the centre takes the residue, w[0] = 4096 - 2 sum(w[1:]), so the taps of a row add up to
    4096 exactly and a constant picture stays as it is.  radius 0..32; 0 gives [4096], the identity.  (For every radius the products
    4096 g[d] / G stay at least 1.5e-3 away from a rounding tie: the table does not depend on the host's libm.)"""
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= 32:
        raise ValueError("blur_taps: radius must be an int in 0..32, got %r" % (radius,))
    if radius == 0:
        return torch.tensor([4096], dtype=torch.int32).to(torch.uint16)
    g = [math.exp(-2.0 * d * d / (radius * radius)) for d in range(radius + 1)]
    total = g[0] + 2.0 * sum(g[1:])
    w = [int(round(4096.0 * v / total)) for v in g[1:]]
    return torch.tensor([4096 - 2 * sum(w)] + w, dtype=torch.int32).to(torch.uint16)


def _backdrop(v, who):
    """A backdrop as the painters take it: a tuple of three ints 0..255, or a contiguous uint8 tensor [Ho, Wo, 3] (kept as handed in)."""
    from .preprocess import YuvFrames
    if isinstance(v, str) and v == "plate":        # the learned background plate (merge.Plate): the video makes the picture
        return v
    if isinstance(v, YuvFrames):
        if len(v) != 1:
            raise ValueError("%s: a backdrop surface must be a YuvFrames of ONE surface, got %d -- slice one, frames[i:i + 1]" % (who, len(v)))
        return v
    if torch.is_tensor(v):
        if v.dtype != torch.uint8 or v.dim() != 3 or v.shape[2] != 3 or v.shape[0] < 1 or v.shape[1] < 1:
            raise ValueError("%s: a backdrop picture must be a uint8 tensor [Ho, Wo, 3] of the output's size, got %s %s -- convert it, "
                             "or give three ints 0..255" % (who, v.dtype, tuple(v.shape)))
        return v
    try:
        t = tuple(v) if not isinstance(v, (str, bytes)) else None
    except TypeError:
        t = None
    if t is None or len(t) != 3 or any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 255 for c in t):
        raise ValueError("%s: backdrop must be three ints 0..255 in the frames' channel order or a uint8 tensor [Ho, Wo, 3], got %r"
                         % (who, v))
    return t


@dataclasses.dataclass
class Style:
    """alpha: weight of the track colour inside a region, 0..1 (the kernel blends with a256 = round(alpha * 256) in 1/256 steps);
    contour: reach in pixels, 0..3, of the full-colour line where a region meets another label (0: none); palette: uint8 [256, 3] in
    the frames' channel order, row = label (None: default_palette()).
    mosaic: None, or what is pixelated instead of tinted (ops.render_mosaic, csrc/render_mosaic.hip): "tracks" -- every track, or with
    `classes` the tracks of those classes, the others tinted as ever; the background stays as decoded -- or "background" -- everything
    but the tracks, which are tinted as alpha / contour say (alpha=0, contour=0: left exactly as decoded).  cell: the side of a mosaic
    cell in output pixels, an even int in 2..64.  classes: None or a collection of class ids >= 0 (kept as a sorted tuple), only with
    mosaic="tracks" or blur="tracks".
    blur: None, or what is blurred instead of tinted (ops.render_blur, csrc/render_blur.hip), with `mosaic`'s meanings: "tracks" --
    every track, or with `classes` the tracks of those classes, the others tinted; the background stays as decoded -- or "background"
    -- everything but the tracks, which are tinted as alpha / contour say.  Not together with a mosaic.  blur_radius: the reach of the
    Gaussian in output pixels, an int in 1..32 (sigma = blur_radius / 2, `blur_taps`; a surface's chroma planes, half as wide, are
    blurred with radius (blur_radius + 1) // 2).  blur_edge: what the blur does at the border of what it blurs.  "bleed": the taps take
    in ALL pixels under the kernel whatever their labels, so a sharp object next to a blurred background smears a halo of blur_radius
    pixels into it and a blurred track takes in its surroundings, as with any plain Gaussian blur.  "stop": the taps weigh only the
    pixels that are blurred themselves and the sum is normalised by the weight it met (ops.render_blur(edge="stop"),
    csrc/render_blur_within.hip), so nothing kept or tinted reaches a blurred pixel; a thin blurred track is then blurred with
    itself only -- a weaker redaction, best used with `grow`.  Only with a blur.
    Annotations (ops.annotate, csrc/annotate.hip: a pass behind whichever painter the fields above choose): box: the thickness in
    pixels, 0..4, of a frame around each track's visible region per frame (0: none); caption: None or which fields are written on a
    plate at the box's top left corner -- "id", "class", "id+class", "id+class+score", "class+score" (`captions`); class_names: None or
    a sequence of names by class id (a caption then shows the name, upper-cased, instead of the number); text_scale: pixels per font
    pixel, 1..4; min_area: regions of fewer pixels get neither box nor caption.
    Trails (ops.render_trails, csrc/paths.hip: a pass between the painter and the annotations, so plates stay legible): trail: 0..64,
    the number of past frames whose centroids (ops.label_centroids: of each track's visible region, the ones of at least min_area
    pixels) are joined to the current frame's by a line in the track's colour, 0: none; trail_width: that line's width in pixels, 1..5.
    replace: None, or what is replaced by `backdrop` through a soft matte (ops.final_matte behind the label map, then ops.render_replace,
    csrc/render_replace.hip, in place of the other painters): "tracks" -- every track, or with `classes` the tracks of those classes,
    the others tinted; the background stays as decoded -- or "background" -- everything but the tracks, which are tinted as alpha /
    contour say (alpha=0, contour=0: left as decoded); with `classes` only the tracks of those classes are kept and every other track
    goes with the background: the virtual-background case.  Not together with a mosaic or a blur.  backdrop: three ints 0..255 in the
    frames' channel order, or a uint8 tensor [Ho, Wo, 3], one picture of the output's size for every frame, or, in a surface=True
    session, a preprocess.YuvFrames of one surface of the session's kind.  matte_gain: in (0, 64],
    the factor on the logit under the matte's sigmoid: above 1 a sharper edge, below 1 a softer one; the matte's 128 level, the hard
    mask's edge, does not move.
    grow: the safety margin of a redaction in output pixels, an int in 0..32 (0: none, and exactly the former launches are made).  Behind
    the label map one ops.grow_labels launch (csrc/grow.hip) makes a grown copy of it and the painter takes that copy: with
    mosaic="tracks" or blur="tracks" the tracks that are pixelated or blurred grow by up to `grow` pixels (a Euclidean disc; where two
    meet, the nearer wins) over the background and over the tinted tracks, so hair, fingers and motion-blurred borders that the mask
    under-covers are redacted too; with mosaic="background", blur="background" or the plain overlay every track grows, so the objects
    keep a sharp margin, or the tint becomes wider (`grows`).  Contours and tints are those of the grown map.  Every other output --
    the label maps, boxes, captions, trails, crops, polygons, mattes, masks -- stays that of the map as the model made it.  Not with
    `replace`: there the matte owns the edge.
    Object removal: backdrop="plate", only with replace="tracks" -- the backdrop is the scene itself, a background plate the video
    learns on the device from the pixels no track covers (merge.Plate, ops.plate_update / ops.plate_picture, csrc/plate.hip; the rule
    is in include/mdqe_hip.h), so the replaced tracks are gone from the picture.  plate_frames: the memory N of the plate's running
    mean in observations, an int in 1..256 (the first N observations of a pixel form their mean, later ones weigh 1 / N).  plate_margin:
    an int in 0..32; a pixel teaches the plate only where no labelled pixel lies within this many output pixels (Euclidean), so an
    object's fringe, which masks under-cover, stays out of it.  plate_reach: an int in 0..32; a pixel that has never been seen free
    takes the nearest seen pixel within this distance, else plate_fill (three ints 0..255 in the frames' channel order).  plate_init:
    None, or an empty-scene shot the plate starts from -- a uint8 tensor [Ho, Wo, 3] of the output's size, or in a surface=True
    session a preprocess.YuvFrames of one surface of the session's kind -- the remedy for a fixed camera whose objects never move
    away.  The state belongs to the video, never to the style: sessions may share a style."""
    alpha: float = 0.5
    contour: int = 1
    palette: torch.Tensor = None
    mosaic: str = None
    cell: int = 16
    classes: tuple = None
    blur: str = None
    blur_radius: int = 8
    box: int = 0
    caption: str = None
    class_names: tuple = None
    text_scale: int = 1
    min_area: int = 0
    trail: int = 0
    trail_width: int = 2
    replace: str = None
    backdrop: object = (0, 255, 0)
    matte_gain: float = 1.0
    grow: int = 0
    blur_edge: str = "bleed"
    plate_frames: int = 64
    plate_margin: int = 4
    plate_reach: int = 16
    plate_fill: tuple = (128, 128, 128)
    plate_init: object = None

    def __post_init__(self):
        for k, lo, hi, what in (("plate_frames", 1, 256, "the memory of the plate's running mean in observations"),
                                ("plate_margin", 0, 32, "how far from any label a pixel must lie to teach the plate, in output pixels"),
                                ("plate_reach", 0, 32, "how far a never-seen pixel looks for a seen one, in output pixels")):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError("overlay style: %s is %s, an int in %d..%d; got %r" % (k, what, lo, hi, v))
        if isinstance(self.grow, bool) or not isinstance(self.grow, int) or not 0 <= self.grow <= 32:
            raise ValueError("overlay style: grow must be an int in 0..32, got %r" % (self.grow,))
        if isinstance(self.trail, bool) or not isinstance(self.trail, int) or not 0 <= self.trail <= 64:
            raise ValueError("overlay style: trail must be an int in 0..64, got %r" % (self.trail,))
        if isinstance(self.trail_width, bool) or not isinstance(self.trail_width, int) or not 1 <= self.trail_width <= 5:
            raise ValueError("overlay style: trail_width must be an int in 1..5, got %r" % (self.trail_width,))
        if isinstance(self.box, bool) or not isinstance(self.box, int) or not 0 <= self.box <= 4:
            raise ValueError("overlay style: box must be an int in 0..4, got %r" % (self.box,))
        if self.caption not in CAPTIONS:
            raise ValueError("overlay style: caption must be one of %s, got %r" % (", ".join(repr(c) for c in CAPTIONS), self.caption))
        if self.class_names is not None:
            try:
                names = tuple(self.class_names) if not isinstance(self.class_names, (str, bytes)) else None
            except TypeError:
                names = None
            if names is None or any(not isinstance(s, str) for s in names):
                raise ValueError("overlay style: class_names must be None or a sequence of strings, got %r" % (self.class_names,))
            self.class_names = names
        if isinstance(self.text_scale, bool) or not isinstance(self.text_scale, int) or not 1 <= self.text_scale <= 4:
            raise ValueError("overlay style: text_scale must be an int in 1..4, got %r" % (self.text_scale,))
        if isinstance(self.min_area, bool) or not isinstance(self.min_area, int) or not 0 <= self.min_area < 2 ** 31:
            raise ValueError("overlay style: min_area must be an int in 0..2^31 - 1, got %r" % (self.min_area,))
        if isinstance(self.alpha, bool) or not isinstance(self.alpha, (int, float)) or not 0.0 <= self.alpha <= 1.0:
            raise ValueError("overlay style: alpha must be a number in 0..1, got %r" % (self.alpha,))
        if isinstance(self.contour, bool) or not isinstance(self.contour, int) or not 0 <= self.contour <= 3:
            raise ValueError("overlay style: contour must be an int in 0..3, got %r" % (self.contour,))
        if self.palette is not None and (not torch.is_tensor(self.palette) or self.palette.dtype != torch.uint8
                                         or tuple(self.palette.shape) != (256, 3)):
            raise ValueError("overlay style: palette must be a uint8 [256, 3] tensor or None")
        if self.mosaic not in (None, "tracks", "background"):
            raise ValueError("overlay style: mosaic must be None, 'tracks' or 'background', got %r" % (self.mosaic,))
        if isinstance(self.cell, bool) or not isinstance(self.cell, int) or not 2 <= self.cell <= 64 or self.cell % 2:
            raise ValueError("overlay style: cell must be an even int in 2..64, got %r" % (self.cell,))
        if self.blur not in (None, "tracks", "background"):
            raise ValueError("overlay style: blur must be None, 'tracks' or 'background', got %r" % (self.blur,))
        if isinstance(self.blur_radius, bool) or not isinstance(self.blur_radius, int) or not 1 <= self.blur_radius <= 32:
            raise ValueError("overlay style: blur_radius must be an int in 1..32, got %r" % (self.blur_radius,))
        if self.blur_edge not in ("bleed", "stop"):
            raise ValueError("overlay style: blur_edge must be 'bleed' or 'stop', got %r" % (self.blur_edge,))
        if self.blur_edge == "stop" and self.blur is None:
            raise ValueError("overlay style: blur_edge='stop' is the edge of a blur -- add blur='tracks' or blur='background', or leave "
                             "blur_edge at 'bleed'; got blur_edge='stop' with blur=None")
        if self.mosaic is not None and self.blur is not None:
            raise ValueError("overlay style: a style has a mosaic or a blur, not both; got mosaic=%r with blur=%r" % (self.mosaic, self.blur))
        if self.replace not in (None, "tracks", "background"):
            raise ValueError("overlay style: replace must be None, 'tracks' or 'background', got %r" % (self.replace,))
        if self.replace is not None and (self.mosaic is not None or self.blur is not None):
            raise ValueError("overlay style: a style has at most one of mosaic, blur and replace -- drop two of them; got mosaic=%r, "
                             "blur=%r, replace=%r" % (self.mosaic, self.blur, self.replace))
        if (isinstance(self.matte_gain, bool) or not isinstance(self.matte_gain, (int, float))
                or not 0.0 < float(self.matte_gain) <= 64.0):
            raise ValueError("overlay style: matte_gain must be a number in (0, 64] (1.0: the model's own sigmoid), got %r" % (self.matte_gain,))
        if self.grow > 0 and self.replace is not None:
            raise ValueError("overlay style: grow is the margin of a mosaic, a blur or the tint; with replace=%r the matte owns the edge "
                             "-- lower matte_gain for a softer, wider edge, or use blur= or mosaic= with grow=%d" % (self.replace, self.grow))
        self.backdrop = _backdrop(self.backdrop, "overlay style")
        if self.plate and self.replace != "tracks":
            raise ValueError("overlay style: backdrop='plate' is the scene behind the tracks, learned where no track is: it goes with "
                             "replace='tracks' only -- set replace='tracks', or give a colour or a picture as the backdrop; got replace=%r"
                             % (self.replace,))
        try:
            fill = tuple(self.plate_fill) if not isinstance(self.plate_fill, (str, bytes)) and not torch.is_tensor(self.plate_fill) else None
        except TypeError:
            fill = None
        if fill is None or len(fill) != 3 or any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 255 for c in fill):
            raise ValueError("overlay style: plate_fill must be three ints 0..255 in the frames' channel order, got %r" % (self.plate_fill,))
        self.plate_fill = fill
        if self.plate_init is not None:
            if not self.plate:
                raise ValueError("overlay style: plate_init is what a background plate starts from -- add replace='tracks', "
                                 "backdrop='plate', or hand the picture in as the backdrop itself; got backdrop=%r"
                                 % (self.backdrop if not torch.is_tensor(self.backdrop) else "a picture",))
            from .preprocess import YuvFrames
            if not torch.is_tensor(self.plate_init) and not isinstance(self.plate_init, YuvFrames):
                raise ValueError("overlay style: plate_init must be None, a uint8 tensor [Ho, Wo, 3] of the output's size or a "
                                 "preprocess.YuvFrames of one surface, got %r" % (self.plate_init,))
            self.plate_init = _backdrop(self.plate_init, "overlay style: plate_init")
        if self.classes is not None:
            try:
                cls = tuple(self.classes) if not isinstance(self.classes, (str, bytes)) else None
            except TypeError:
                cls = None
            if cls is None or any(isinstance(c, bool) or not isinstance(c, int) or c < 0 for c in cls):
                raise ValueError("overlay style: classes must be None or a collection of ints >= 0, got %r" % (self.classes,))
            if self.mosaic != "tracks" and self.blur != "tracks" and self.replace is None:
                raise ValueError("overlay style: classes selects the tracks that mosaic='tracks' pixelates or blur='tracks' blurs; got "
                                 "classes with mosaic=%r, blur=%r" % (self.mosaic, self.blur))
            self.classes = tuple(sorted(set(cls)))

    @property
    def a256(self):
        return int(round(self.alpha * 256))

    @property
    def annotates(self):
        """Whether an annotation pass follows the painter (with the defaults: no, and exactly the painter's launches are made)."""
        return self.box > 0 or self.caption is not None

    @property
    def trails(self):
        """Whether a trail pass runs between the painter and the annotations (with the defaults: no, and exactly the painter's launches
        are made)."""
        return self.trail > 0

    @property
    def plate(self):
        """Whether the backdrop is the learned background plate (merge.Plate); with any other backdrop nothing of it is made or launched."""
        return isinstance(self.backdrop, str) and self.backdrop == "plate"

    def plate_fill_on(self, device):
        """plate_fill on `device`, uint8 [3] (cached per device)."""
        return self._cached_on("_plate_fill_on", (str(device),), lambda: torch.tensor(self.plate_fill, dtype=torch.uint8))

    def plate_fill_yuv_on(self, device, fmt, matrix, full_range, order):
        """`backdrop_yuv(plate_fill, ...)` on `device`, uint16 [3] (cached per device and kind of surface)."""
        return self._cached_on("_plate_fill_yuv_on", (str(device), fmt, matrix, bool(full_range), order),
                               lambda: backdrop_yuv(self.plate_fill, fmt, matrix, bool(full_range), order))

    def plate_init_on(self, device):
        """plate_init on `device` (cached per device): a contiguous uint8 [Ho, Wo, 3] picture, or a YuvFrames of one surface."""
        from .preprocess import YuvFrames
        if isinstance(self.plate_init, YuvFrames):
            return self._cached_on("_plate_init_on", (str(device),), lambda: self.plate_init, YuvFrames.to)
        return self._cached_on("_plate_init_on", (str(device),), lambda: self.plate_init)

    def _cached_on(self, slot, key, make, to=lambda t, device: t.contiguous().to(device)):
        """What `make()` gives on the host, on the device key[0]: made and moved there once per `key` -- one tiny upload per session, not
        per window.  `to(made, device)` moves it: a small table (a tensor) by default."""
        cache = self.__dict__.setdefault(slot, {})
        if key not in cache:
            cache[key] = to(make(), key[0])
            if cache[key].is_cuda:                 # later windows read it on other streams: the one upload is complete before it is handed out
                torch.cuda.current_stream(cache[key].device).synchronize()
        return cache[key]

    def font_on(self, device):
        """`default_font()` on `device` (cached per device)."""
        return self._cached_on("_font_on", (str(device),), default_font)

    def ink_on(self, device):
        """`ink` of the palette on `device` (cached per device)."""
        return self._cached_on("_ink_on", (str(device),), lambda: ink(default_palette() if self.palette is None else self.palette))

    def ink_yuv_on(self, device, fmt, matrix, full_range, order):
        """`palette_yuv(ink(palette), ...)` on `device` (cached per device and kind of surface, as `palette_yuv_on` is)."""
        return self._cached_on("_ink_yuv_on", (str(device), fmt, matrix, bool(full_range), order),
                               lambda: palette_yuv(ink(default_palette() if self.palette is None else self.palette), fmt, matrix,
                                                   bool(full_range), order))

    def captions_on(self, device, cls_probs, n):
        """`captions` of a window on `device`, or None without a caption: built from the window's class rows and uploaded, 8 KB per
        window (as `actions_on` does with `classes`)."""
        return None if self.caption is None else captions(self, cls_probs, n).to(device)

    def actions(self, cls_probs=None):
        """The per-label action table of ops.render_mosaic / ops.render_blur / ops.render_replace, uint8 [256] on the host (0 keep, 1 tint,
        2 mosaic, 3 blur, 4 replace; entry 0 is the background's), a pure function.  With r = 2 for a mosaic, 3 for a blur and 4 for a
        replacement: none of them: [0, 1, 1, ...] (the plain overlay); "background": [r, 1, 1, ...]; "tracks": [0, r, r, ...], or with
        `classes`, from the window's class rows cls_probs [n, K] (win.cls_probs): label t + 1 gets r when the first maximum of row t
        is a class in `classes` and 1 otherwise, and so do the labels above n.  replace="background" with `classes` (the only
        "background" that takes them): [4, then 1 for the tracks of the listed classes and 4 for the others, 4 above n]."""
        what, r = (self.replace, 4) if self.replace is not None else (self.blur, 3) if self.blur is not None else (self.mosaic, 2)
        act = torch.ones(256, dtype=torch.uint8)
        act[0] = r if what == "background" else 0
        if what == "tracks" and self.classes is None:
            act[1:] = r
        elif what == "tracks" or (r == 4 and self.classes is not None):
            if not torch.is_tensor(cls_probs) or cls_probs.dim() != 2:
                raise ValueError("overlay style: a %s of classes needs the window's class rows [n, K], got %r"
                                 % ({2: "mosaic", 3: "blur", 4: "replacement"}[r], type(cls_probs).__name__))
            # replace="background" with classes: the listed tracks are kept (tinted), every other label goes with the background
            hit_as, miss_as = (1, 4) if what == "background" else (r, 1)
            act[1:] = miss_as
            n = min(int(cls_probs.shape[0]), 255)
            if n and cls_probs.shape[1]:
                rows = cls_probs[:n].detach().cpu()
                first = rows.argmax(1)                  # (of several maxima the first: torch.argmax's rule)
                hit = torch.isin(first, torch.tensor(self.classes, dtype=first.dtype))
                act[1:n + 1] = torch.where(hit, hit_as, miss_as).to(torch.uint8)
        return act

    def grows(self, cls_probs=None):
        """The table of ops.grow_labels, uint8 [256] on the host, a pure function of `actions(cls_probs)`: entry l says whether label l
        grows by the style's margin.  With mosaic="tracks" or blur="tracks": exactly the labels whose action is the redaction (2 or 3)
        -- with `classes` only those tracks, and they grow over the tinted ones; with mosaic="background", blur="background" or the
        plain overlay: every label >= 1.  Entry 0 is 0: the background never grows."""
        act = self.actions(cls_probs)
        what = self.blur if self.blur is not None else self.mosaic
        g = ((act == 2) | (act == 3)) if what == "tracks" else torch.ones(256, dtype=torch.bool)
        g[0] = False
        return g.to(torch.uint8)

    def grows_on(self, device, cls_probs=None):
        """`grows` on `device`: cached per device where the table does not depend on the window (no `classes`), as `actions_on` is."""
        if self.classes is not None:
            return self.grows(cls_probs).to(device)
        return self._cached_on("_grow_on", (str(device),), self.grows)

    def takes(self, cls_probs=None):
        """The matte's row table of ops.final_matte for a replace style, uint8 [256] on the host, from `actions(cls_probs)`: entry l says
        whether the track of label l takes part in the matte -- "background": the tracks that are kept (action != 4, labels >= 1: the
        matte is the foreground); "tracks": the tracks that are replaced (action == 4: the matte covers them).  Entry 0 is 0 (unused)."""
        if self.replace is None:
            raise ValueError("overlay style: takes() is the matte's table of a style with replace='tracks' or 'background'")
        act = self.actions(cls_probs)
        take = (act != 4) if self.replace == "background" else (act == 4)
        take[0] = False
        return take.to(torch.uint8)

    def takes_on(self, device, cls_probs=None):
        """`takes` on `device`: cached per device where the table does not depend on the window (no `classes`), as `actions_on` is."""
        if self.classes is not None:
            return self.takes(cls_probs).to(device)
        return self._cached_on("_take_on", (str(device),), self.takes)

    def backdrop_on(self, device):
        """The backdrop on `device`, contiguous uint8 [3] or [Ho, Wo, 3] (cached per device, as the palette is)."""
        return self._cached_on("_backdrop_on", (str(device),),
                               lambda: self.backdrop if torch.is_tensor(self.backdrop) else torch.tensor(self.backdrop, dtype=torch.uint8))

    def backdrop_yuv_on(self, device, fmt, matrix, full_range, order):
        """The backdrop of a surface session on `device` (cached per device and kind of surface): `backdrop_yuv` of a colour, or the
        backdrop surface itself moved there."""
        from .preprocess import YuvFrames
        key = (str(device), fmt, matrix, bool(full_range), order)
        if not isinstance(self.backdrop, YuvFrames):
            return self._cached_on("_backdrop_yuv_on", key, lambda: backdrop_yuv(self.backdrop, fmt, matrix, bool(full_range), order))
        return self._cached_on("_backdrop_yuv_on", key, lambda: self.backdrop, YuvFrames.to)

    def actions_on(self, device, cls_probs=None):
        """`actions` on `device`: cached per device as the palette is where the table does not depend on the window (no `classes`);
        with `classes` built from the window's class rows and uploaded, 256 bytes per window."""
        if self.classes is not None:
            return self.actions(cls_probs).to(device)
        return self._cached_on("_act_on", (str(device),), self.actions)

    def taps_on(self, device):
        """`blur_taps(blur_radius)` on `device` (cached per device, as `palette_on` keeps the palette)."""
        return self._cached_on("_taps_on", (str(device), self.blur_radius), lambda: blur_taps(self.blur_radius))

    def taps_c_on(self, device):
        """The chroma planes' taps of a surface, `blur_taps((blur_radius + 1) // 2)`, on `device` (cached per device)."""
        return self._cached_on("_taps_c_on", (str(device), self.blur_radius), lambda: blur_taps((self.blur_radius + 1) // 2))

    def palette_on(self, device):
        """The palette on `device`, contiguous (cached per device)."""
        return self._cached_on("_on", (str(device),), lambda: default_palette() if self.palette is None else self.palette)

    def palette_yuv_on(self, device, fmt, matrix, full_range, order):
        """`palette_yuv` of the palette on `device` (cached per device and kind of surface, as `palette_on` is)."""
        return self._cached_on("_yuv_on", (str(device), fmt, matrix, bool(full_range), order),
                               lambda: palette_yuv(default_palette() if self.palette is None else self.palette, fmt, matrix,
                                                   bool(full_range), order))


@dataclasses.dataclass(frozen=True)
class Matte:
    """The soft matte as a video output of its own (model.matte_output, online_video(matte=...)), beside any other output: per frame one
    uint8 plane, rint(255 * sigmoid(gain * the largest up-sampled logit among the window's tracks)), held at >= 128 exactly where one
    of their final masks is set (ops.final_matte, csrc/final_mask.hip) -- the union matte of the tracks, what compositing and
    rotoscoping take.  classes: None (every track) or a collection of class ids >= 0 (kept as a sorted tuple): only the tracks whose
    window class row has its first maximum in one of them; gain: in (0, 64], above 1 a sharper edge, below 1 a softer one."""
    classes: tuple = None
    gain: float = 1.0

    def __post_init__(self):
        if isinstance(self.gain, bool) or not isinstance(self.gain, (int, float)) or not 0.0 < float(self.gain) <= 64.0:
            raise ValueError("matte: gain must be a number in (0, 64] (1.0: the model's own sigmoid), got %r" % (self.gain,))
        if self.classes is not None:
            try:
                cls = tuple(self.classes) if not isinstance(self.classes, (str, bytes)) else None
            except TypeError:
                cls = None
            if cls is None or any(isinstance(c, bool) or not isinstance(c, int) or c < 0 for c in cls):
                raise ValueError("matte: classes must be None or a collection of ints >= 0, got %r" % (self.classes,))
            object.__setattr__(self, "classes", tuple(sorted(set(cls))))

    def takes(self, cls_probs=None):
        """ops.final_matte's row table, uint8 [256] on the host by label, or None without `classes` (every row takes part): label
        t + 1 is 1 when the first maximum of row t of the window's class rows cls_probs [n, K] is a listed class."""
        if self.classes is None:
            return None
        if not torch.is_tensor(cls_probs) or cls_probs.dim() != 2:
            raise ValueError("matte: classes need the window's class rows [n, K], got %r" % type(cls_probs).__name__)
        take = torch.zeros(256, dtype=torch.uint8)
        n = min(int(cls_probs.shape[0]), 255)
        if n and cls_probs.shape[1]:
            first = cls_probs[:n].detach().cpu().argmax(1)
            take[1:n + 1] = torch.isin(first, torch.tensor(self.classes, dtype=first.dtype)).to(torch.uint8)
        return take


@dataclasses.dataclass(frozen=True)
class Crops:
    """Per-track crops as a video output (model.crop_output, online_video(crops=...)): one fixed-size picture per track and frame, cut
    from the frames handed in and resized on the device (ops.track_crops, csrc/crops.hip) from the label map's visible regions.
    size: (height, width) of a chip, each 1..512; pad: how far the box grows per side, as a fraction 0..1 of its width / height (the
    kernel uses pad256 = rint(pad * 256), clamped to the picture); cutout: only the pixels the track owns count, the rest of a chip is
    `fill`; fill: three ints 0..255 in the frames' channel order -- the colour of a chip without a box and of what a cutout leaves
    out; min_area: visible regions of fewer pixels give a chip of `fill`; every >= 1: the video frames f with f % every == 0 are taken
    (the buffers shrink by that factor)."""
    size: tuple = (128, 64)
    pad: float = 0.0
    cutout: bool = False
    fill: tuple = (0, 0, 0)
    min_area: int = 0
    every: int = 1

    def __post_init__(self):
        def ints(v, k, lo, hi):
            try:
                t = tuple(v) if not isinstance(v, (str, bytes)) else None
            except TypeError:
                t = None
            return t if t is not None and len(t) == k and all(not isinstance(x, bool) and isinstance(x, int) and lo <= x <= hi for x in t) else None
        size, fill = ints(self.size, 2, 1, 512), ints(self.fill, 3, 0, 255)
        if size is None:
            raise ValueError("crops: size must be (height, width), ints in 1..512, got %r" % (self.size,))
        if fill is None:
            raise ValueError("crops: fill must be three ints in 0..255 (the frames' channel order), got %r" % (self.fill,))
        if isinstance(self.pad, bool) or not isinstance(self.pad, (int, float)) or not 0.0 <= self.pad <= 1.0:
            raise ValueError("crops: pad must be a number in 0..1 (a fraction of the box per side), got %r" % (self.pad,))
        if not isinstance(self.cutout, bool):
            raise ValueError("crops: cutout must be a bool, got %r" % (self.cutout,))
        if isinstance(self.min_area, bool) or not isinstance(self.min_area, int) or not 0 <= self.min_area < 2 ** 31:
            raise ValueError("crops: min_area must be an int in 0..2^31 - 1, got %r" % (self.min_area,))
        if isinstance(self.every, bool) or not isinstance(self.every, int) or self.every < 1:
            raise ValueError("crops: every must be an int >= 1, got %r" % (self.every,))
        object.__setattr__(self, "size", size)
        object.__setattr__(self, "fill", fill)

    @property
    def pad256(self):
        return int(round(self.pad * 256))

    def first_in(self, f0):
        """The first frame taken of a window (or a store piece) that starts at video frame f0, relative to it."""
        return (-int(f0)) % self.every

    def taken(self, f0, f1):
        """The video frames taken among [f0, f1)."""
        return list(range(int(f0) + self.first_in(f0), int(f1), self.every))

    def count(self, n_frames):
        """Lc = ceil(n_frames / every): the frames taken of a whole video."""
        return -(-int(n_frames) // self.every)
