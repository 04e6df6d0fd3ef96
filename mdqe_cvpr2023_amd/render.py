"""How an overlay is painted (model.overlay_output, online_video(emit="overlay")): the palette and the style.  The painting itself is
ops.render_overlay (csrc/render.hip) behind the label map; merge.overlay_frames puts the two together for a tracker window.

A track's colour depends only on its tracker row (label = row + 1), so it keeps its colour across windows and pushes."""
import dataclasses

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


@dataclasses.dataclass
class Style:
    """alpha: weight of the track colour inside a region, 0..1 (the kernel blends with a256 = round(alpha * 256) in 1/256 steps);
    contour: reach in pixels, 0..3, of the full-colour line where a region meets another label (0: none); palette: uint8 [256, 3] in
    the frames' channel order, row = label (None: default_palette())."""
    alpha: float = 0.5
    contour: int = 1
    palette: torch.Tensor = None

    def __post_init__(self):
        if isinstance(self.alpha, bool) or not isinstance(self.alpha, (int, float)) or not 0.0 <= self.alpha <= 1.0:
            raise ValueError("overlay style: alpha must be a number in 0..1, got %r" % (self.alpha,))
        if isinstance(self.contour, bool) or not isinstance(self.contour, int) or not 0 <= self.contour <= 3:
            raise ValueError("overlay style: contour must be an int in 0..3, got %r" % (self.contour,))
        if self.palette is not None and (not torch.is_tensor(self.palette) or self.palette.dtype != torch.uint8
                                         or tuple(self.palette.shape) != (256, 3)):
            raise ValueError("overlay style: palette must be a uint8 [256, 3] tensor or None")

    @property
    def a256(self):
        return int(round(self.alpha * 256))

    def palette_on(self, device):
        """The palette on `device`, contiguous (cached per device: one tiny upload per session, not per window)."""
        cache = self.__dict__.setdefault("_on", {})
        key = str(device)
        if key not in cache:
            pal = default_palette() if self.palette is None else self.palette
            cache[key] = pal.contiguous().to(device)
            if cache[key].is_cuda:                 # later windows read it on other streams: the one upload is complete before it is handed out
                torch.cuda.current_stream(cache[key].device).synchronize()
        return cache[key]
