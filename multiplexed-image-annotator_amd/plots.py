"""Host side of the two per-cell-type plots (Annotator.generate_heatmap, model.py:700-741; Annotator.cell_type_composition,
model.py:861-912): the wedge boundaries of the pie, the texts, the CSVs, and the PIL composition around the rectangles the GPU rasterises
(ops.heatmap_raster, ops.pie_raster) -- labels in PIL's built-in font, a colour bar from the same look-up table, a legend of swatches.
No matplotlib or seaborn."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

WHITE = (255, 255, 255)
BLACK = (0, 0, 0)
PAD = 6               # pixels between a text and what it labels
BAR_GAP = 16          # between the heat map and its colour bar
BAR_WIDTH = 16
SWATCH = 12           # side of a legend swatch
LEGEND_LINE = 16      # height of a legend line


# ---- pie ------------------------------------------------------------------------------------------------------------------------------------
def pie_wedges(counts: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """(kept, rays): the indices of the wedges that are not empty, in order, and the (len(kept) - 1, 2) fp64 (cos, sin) of the boundaries between
    them -- wedge k ends at the angle 2 pi (n_0 + ... + n_k) / N from 3 o'clock, counter-clockwise (matplotlib's ax.pie); the closing boundary at
    2 pi is dropped.  No cells at all: no wedge."""
    counts = np.asarray(counts, dtype=np.int64)
    kept = np.nonzero(counts > 0)[0]
    if len(kept) == 0:
        return kept, np.zeros((0, 2), dtype=np.float64)
    cum = np.cumsum(counts[kept])[:-1].astype(np.float64)
    theta = 2.0 * np.pi * (cum / float(counts.sum()))
    return kept, np.stack([np.cos(theta), np.sin(theta)], axis=1).reshape(-1, 2)


def legend_texts(names: Sequence[str], counts: Sequence[int], reduction: bool = True) -> List[str]:
    """model.py:876 / 904: f"{name} ({v * 100:.2f} %)" with v = count / N -- or, with reduction=False, the raw count, which the reference
    multiplies by 100 all the same (restated, not repaired)."""
    total = int(sum(int(c) for c in counts))
    out = []
    for name, c in zip(names, counts):
        v = int(c)
        if reduction:
            v = v / total if total else 0.0
        out.append(f"{name} ({v * 100:.2f} %)")
    return out


def composition_csv(names: Sequence[str], counts: Sequence[int]) -> str:
    total = int(sum(int(c) for c in counts))
    lines = ["cell_type,cells,fraction"]
    for name, c in zip(names, counts):
        lines.append(f"{name},{int(c)},{(int(c) / total if total else 0.0):.17g}")
    return "\n".join(lines) + "\n"


def heatmap_csv(names: Sequence[str], markers: Sequence[str], means: np.ndarray, counts: Sequence[int]) -> str:
    """one row per cell type: its name, the mean of every channel with 17 significant digits (the text parses back to the same doubles), its cells"""
    lines = ["cell_type," + ",".join(str(m) for m in markers) + ",cells"]
    for name, row, c in zip(names, np.asarray(means, dtype=np.float64), counts):
        lines.append(f"{name}," + ",".join(f"{v:.17g}" for v in row.tolist()) + f",{int(c)}")
    return "\n".join(lines) + "\n"


# ---- drawing --------------------------------------------------------------------------------------------------------------------------------
def _font():
    from PIL import ImageFont
    return ImageFont.load_default()


def _text_size(font, text: str) -> Tuple[int, int]:
    l, t, r, b = font.getbbox(text)
    return int(r), int(b)


def _text_image(font, text: str):
    from PIL import Image, ImageDraw
    w, h = _text_size(font, text)
    img = Image.new("RGB", (max(w, 1), max(h, 1)), WHITE)
    ImageDraw.Draw(img).text((0, 0), text, fill=BLACK, font=font)
    return img


def heatmap_layout(row_labels: Sequence[str], col_labels: Sequence[str], cell: int, scale_texts: Sequence[str]) -> Dict[str, int]:
    """where the pieces of the figure go: the data rectangle starts at (top, left)"""
    font = _font()
    left = max(_text_size(font, str(s))[0] for s in row_labels) + 2 * PAD
    bottom = max(_text_size(font, str(s))[0] for s in col_labels) + 2 * PAD
    right = BAR_GAP + BAR_WIDTH + max(_text_size(font, s)[0] for s in scale_texts) + 2 * PAD
    top = PAD + _text_size(font, "0")[1]
    h, w = len(row_labels) * cell, len(col_labels) * cell
    return {"top": top, "left": left, "height": top + h + bottom, "width": left + w + right, "rect_height": h, "rect_width": w}


def heatmap_figure(rect: np.ndarray, lut: np.ndarray, vmin: float, vmax: float, row_labels: Sequence[str], col_labels: Sequence[str], cell: int):
    """PIL image: the (T cell, C cell, 3) data rectangle with its row labels on the left, the column labels turned by 90 degrees underneath and a
    colour bar with vmax / vmin on the right"""
    from PIL import Image
    font = _font()
    scale = [f"{vmax:.4g}", f"{vmin:.4g}"]
    lay = heatmap_layout(row_labels, col_labels, cell, scale)
    top, left, h, w = lay["top"], lay["left"], lay["rect_height"], lay["rect_width"]
    fig = Image.new("RGB", (lay["width"], lay["height"]), WHITE)
    fig.paste(Image.fromarray(np.ascontiguousarray(rect)), (left, top))
    for t, s in enumerate(row_labels):
        img = _text_image(font, str(s))
        fig.paste(img, (left - PAD - img.width, top + t * cell + max((cell - img.height) // 2, 0)))
    for j, s in enumerate(col_labels):
        img = _text_image(font, str(s)).rotate(90, expand=True)
        fig.paste(img, (left + j * cell + max((cell - img.width) // 2, 0), top + h + PAD))
    # the bar: the table's 256 colours, the highest on top
    idx = 255 - (np.arange(h, dtype=np.int64) * 256) // h
    bar = np.repeat(np.asarray(lut, dtype=np.uint8)[idx][:, None, :], BAR_WIDTH, axis=1)
    x0 = left + w + BAR_GAP
    fig.paste(Image.fromarray(np.ascontiguousarray(bar)), (x0, top))
    hi, lo = _text_image(font, scale[0]), _text_image(font, scale[1])
    fig.paste(hi, (x0 + BAR_WIDTH + PAD, top - hi.height // 2))
    fig.paste(lo, (x0 + BAR_WIDTH + PAD, top + h - lo.height // 2 - 1))
    return fig, lay


def pie_layout(texts: Sequence[str], canvas: int) -> Dict[str, int]:
    """the disc canvas starts at (top, 0); the legend stands to its right, centred vertically (the reference's loc="center left")"""
    font = _font()
    legend_h = len(texts) * LEGEND_LINE + 2 * PAD
    legend_w = PAD + SWATCH + PAD + max([_text_size(font, s)[0] for s in texts] + [0]) + PAD
    height = max(canvas, legend_h)
    return {"top": (height - canvas) // 2, "left": 0, "height": height, "width": canvas + legend_w, "legend_top": (height - legend_h) // 2 + PAD}


def pie_figure(disc: np.ndarray, texts: Sequence[str], colours: Sequence[Sequence[int]]):
    """PIL image: the (canvas, canvas, 3) disc and, beside it, one swatch and text per cell type"""
    from PIL import Image, ImageDraw
    font = _font()
    canvas = int(disc.shape[0])
    lay = pie_layout(texts, canvas)
    fig = Image.new("RGB", (lay["width"], lay["height"]), WHITE)
    fig.paste(Image.fromarray(np.ascontiguousarray(disc)), (lay["left"], lay["top"]))
    draw = ImageDraw.Draw(fig)
    for k, (s, rgb) in enumerate(zip(texts, colours)):
        y = lay["legend_top"] + k * LEGEND_LINE
        x = canvas + PAD
        draw.rectangle([x, y, x + SWATCH - 1, y + SWATCH - 1], fill=tuple(int(v) for v in rgb), outline=BLACK)
        draw.text((x + SWATCH + PAD, y), s, fill=BLACK, font=font)
    return fig, lay
