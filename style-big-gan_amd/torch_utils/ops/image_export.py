"""The image writers' arithmetic as HIP kernels (csrc/image_export.hip): float images -> uint8 in a grid canvas, and the truncated,
style-mixed latent table of the style matrix.

Two quantisation rules, because the reference uses both and they differ on ties:
* ``grid``  -- ``save_image_grid`` (train_parts/trainers.py:102-106): ``rint((x - lo) * (255 / (hi - lo))).clip(0, 255)``;
* ``clamp`` -- stylegan2ada/generate.py:98,120 and style_mixing.py:79,88: ``(x * 127.5 + 128).clamp(0, 255)`` truncated.
Device tensors run the kernels; CPU tensors run the reference's own formulas (numpy for ``grid``, torch for ``clamp``), so the plumbing
is testable without a GPU.  On the device an unsupported input is an error, never a quiet torch fallback.  Non-finite values, which
the reference leaves undefined, are defined here on both paths: NaN writes 0, +-inf clamp.
"""
import numpy as np
import torch

from ... import _lib

RULES = tuple(_lib.QUANT_RULES)


def _check_images(img, rule, drange, what):
    if rule not in _lib.QUANT_RULES:
        raise RuntimeError(f"{what}: unknown rule {rule!r} (one of {RULES})")
    if img.ndim != 4 or img.shape[1] not in (1, 3) or img.numel() == 0:
        raise RuntimeError(f"{what}: expects images [N, C, H, W] with C = 1 or 3, got {list(img.shape)}")
    if img.dtype != torch.float32:
        raise RuntimeError(f"{what}: expects float32 images, got {img.dtype}")
    if rule == "grid":
        if drange is None or len(drange) != 2 or not float(drange[1]) != float(drange[0]):
            raise RuntimeError(f"{what}: the grid rule needs drange=(lo, hi) with hi != lo, got {drange}")
    elif drange is not None:
        raise RuntimeError(f"{what}: the clamp rule has a fixed range; drange must be None")


def quantize_reference(img, rule, drange=None):
    """CPU float32 [N, C, H, W] -> uint8 [N, H, W, C] by the reference's expressions"""
    if rule == "grid":
        lo, hi = drange
        v = np.asarray(img.detach().numpy(), dtype=np.float32)
        v = (v - lo) * (255 / (hi - lo))
        v = np.where(np.isnan(v), np.float32(0), v)
        v = np.rint(v).clip(0, 255).astype(np.uint8)
        return torch.from_numpy(np.ascontiguousarray(v.transpose(0, 2, 3, 1)))
    v = img.detach().permute(0, 2, 3, 1) * 127.5 + 128
    v = torch.where(v.isnan(), torch.zeros_like(v), v)
    return v.clamp(0, 255).to(torch.uint8).contiguous()


def tile(img, grid_size, rule, drange=None, canvas=None, cell0=0):
    """images [N, C, H, W] -> the HWC canvas uint8 [gh * H, gw * W, C] with image n in cell `cell0 + n` (row-major cells, `grid_size` =
    (gw, gh) as the reference passes it).  `canvas`: filled in place (cells outside [cell0, cell0 + N) keep their bytes) or, when None,
    allocated zeroed on the images' device."""
    what = "image_export tile"
    _check_images(img, rule, drange, what)
    gw, gh = int(grid_size[0]), int(grid_size[1])
    N, C, H, W = img.shape
    cell0 = int(cell0)
    if gw < 1 or gh < 1 or cell0 < 0 or cell0 + N > gw * gh:
        raise RuntimeError(f"{what}: cells [{cell0}, {cell0 + N}) do not fit a {gw} x {gh} grid")
    if canvas is None:
        canvas = torch.zeros([gh * H, gw * W, C], dtype=torch.uint8, device=img.device)
    if canvas.device != img.device:
        raise RuntimeError(f"{what}: images on {img.device}, canvas on {canvas.device}")
    if canvas.dtype != torch.uint8 or tuple(canvas.shape) != (gh * H, gw * W, C) or not canvas.is_contiguous():
        raise RuntimeError(f"{what}: the canvas must be a dense uint8 [{gh * H}, {gw * W}, {C}], got {canvas.dtype} {list(canvas.shape)}")
    if img.device.type != "cuda":
        q = quantize_reference(img, rule, drange)
        for n in range(N):
            gy, gx = divmod(cell0 + n, gw)
            canvas[gy * H:(gy + 1) * H, gx * W:(gx + 1) * W] = q[n]
        return canvas
    img = img.detach()
    lo, scale = (float(np.float32(drange[0])), float(np.float32(255 / (drange[1] - drange[0])))) if rule == "grid" else (0.0, 1.0)
    sn, sc, sh, sw = img.stride()
    _lib.check(_lib.load().sbg_img_quantize_tile(img.data_ptr(), canvas.data_ptr(), N, C, H, W, sn, sc, sh, sw, gw, gh, cell0,
                                                 _lib.QUANT_RULES[rule], lo, scale, _lib.stream_ptr(img.device)), "sbg_img_quantize_tile")
    return canvas


def quantize(img, rule, drange=None):
    """images [N, C, H, W] -> uint8 [N, H, W, C] (a one-column grid of N cells)"""
    _check_images(img, rule, drange, "image_export quantize")
    N, C, H, W = img.shape
    return tile(img, (1, N), rule, drange).reshape(N, H, W, C)


def truncate_mix_reference(ws, w_avg, truncation_psi, rows, cols, col_styles):
    """the reference's statements (style_mixing.py:74, 85-86) for every (row, column) pair"""
    t = w_avg + (ws - w_avg) * truncation_psi
    out = []
    for r in rows:
        for c in cols:
            w = t[r].clone()
            w[col_styles] = t[c][col_styles]
            out.append(w)
    return torch.stack(out)


def truncate_mix(ws, w_avg, truncation_psi, rows, cols, col_styles):
    """mapped latents ws [S, L, D], w_avg [D] -> [R * Cn, L, D]: row r * Cn + c is the truncated latent of `rows[r]` with the layers
    in `col_styles` taken from the truncated latent of `cols[c]`; truncation is w_avg + (ws - w_avg) * psi in that order
    (style_mixing.py:74).  `rows`, `cols`: indices into ws; `col_styles`: layer indices (an empty list mixes nothing, so
    rows = range(S), cols = [0] gives the truncated table itself)."""
    what = "image_export truncate_mix"
    if ws.ndim != 3 or w_avg.shape != ws.shape[2:] or ws.numel() == 0:
        raise RuntimeError(f"{what}: expects ws [S, L, D] and w_avg [D], got {list(ws.shape)} and {list(w_avg.shape)}")
    if ws.dtype != torch.float32 or w_avg.dtype != torch.float32:
        raise RuntimeError(f"{what}: expects float32, got {ws.dtype} and {w_avg.dtype}")
    if ws.device != w_avg.device:
        raise RuntimeError(f"{what}: ws on {ws.device}, w_avg on {w_avg.device}")
    S, L, D = ws.shape
    rows, cols, col_styles = [int(i) for i in rows], [int(i) for i in cols], [int(i) for i in col_styles]
    if not rows or not cols or any(not 0 <= i < S for i in rows + cols):
        raise RuntimeError(f"{what}: rows and cols must be non-empty lists of indices in [0, {S})")
    if any(not -L <= i < L for i in col_styles):
        raise IndexError(f"{what}: a layer of col_styles is out of range for {L} layers")
    col_styles = [i % L for i in col_styles]
    psi = float(truncation_psi)
    if ws.device.type != "cuda":
        return truncate_mix_reference(ws.detach(), w_avg.detach(), psi, rows, cols, col_styles)
    ws, w_avg = ws.detach().contiguous(), w_avg.detach().contiguous()
    mask = [0] * L
    for i in col_styles:
        mask[i] = 1
    table = torch.tensor(rows + cols + mask, dtype=torch.int32).to(ws.device)
    out = torch.empty([len(rows) * len(cols), L, D], dtype=torch.float32, device=ws.device)
    p = table.data_ptr()
    _lib.check(_lib.load().sbg_ws_truncate_mix(ws.data_ptr(), w_avg.data_ptr(), psi, p, p + 4 * len(rows), p + 4 * (len(rows) + len(cols)),
                                               out.data_ptr(), S, L, D, len(rows), len(cols), _lib.stream_ptr(ws.device)), "sbg_ws_truncate_mix")
    return out
