"""Image scores on the GPU: PSNR, L1 and SSIM of rendered views (cnerf_image_metrics, csrc/metrics.hip), and the CLIP scores of an edit.

The reference's evaluate loop feeds numpy arrays to a host-side PSNR meter (nerf/utils_init_nerf.py:673-779) and has no SSIM; here one fused
kernel pass returns per-image float64 sums and this module derives the scores from them in float64.

SSIM definition (libraries differ, so it is written down; include/customnerf_hip.h carries the same text, tests/ssim_restatement.py restates
it in NumPy): Wang et al. 2004 with L = 1, K1 = 0.01, K2 = 0.03; an 11-tap Gaussian window of sigma 1.5 whose weights are computed in float64
and normalised to sum 1, applied separably over the VALID region only — the map is (H - 10) x (W - 10) per channel, no padding; population
moments, sigma_ab = E[ab] - E[a]E[b]; an image's SSIM is the mean of the map over valid pixels and channels.  With a mask a pixel counts for
mse / l1 when its mask value is nonzero, and a window counts for ssim when its CENTRE pixel does.  An image with nothing counted gives nan
and a count of 0: a defined result, not an error.  H or W below 11 raises ValueError.  The five window moments are accumulated in float64
(DESIGN.md section 4d has the numbers behind that decision), so identical images score exactly ssim 1 and psnr inf, and every result is
bit-reproducible from run to run.

quantize=True scores what written 8-bit files hold: both images first go through floor(clamp(v, 0, 1) * 255) / 255 (float32) — the
reference's truncation `(pred * 255).astype(np.uint8)` (utils_init_nerf.py:550) plus a clamp, the rule the trainers' test() writes frames by.
"""
import torch

from ._lib import lib, check, ptr, stream, require_cuda, dtype_id, query_u64

WINDOW = 11                      # taps of the Gaussian window; the map loses WINDOW - 1 rows and columns


def _as_batch(t, what):
    if not torch.is_tensor(t):
        raise TypeError(f"image_metrics: {what} must be a tensor")
    require_cuda(t)
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise ValueError(f"image_metrics: {what} must be [B, H, W, C] or [H, W, C], got {tuple(t.shape)}")
    return t


def image_metrics(pred, target, mask=None, quantize=False, want_map=False):
    """pred, target: CUDA tensors [B, H, W, C] or [H, W, C], float32 or float16 (both the same), C in {1, 3}, values nominally in [0, 1];
    mask: None or [B, H, W] / [H, W] (any real dtype or bool; nonzero = the pixel counts).  Non-contiguous tensors are made contiguous.
    -> dict of [B] float64 CUDA tensors: 'mse', 'l1', 'psnr' (= 10 log10(1 / mse), inf at mse == 0), 'ssim', 'n_pixels' (counted
    pixel-channels), 'n_windows' (counted window-channels), and with want_map 'ssim_map' [B, H - 10, W - 10, C] float32 (the whole map,
    whatever the mask says).  The module docstring defines SSIM and `quantize`.  Runs on the current stream, no host sync."""
    pred, target = _as_batch(pred, "pred"), _as_batch(target, "target")
    if pred.shape != target.shape:
        raise ValueError(f"image_metrics: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if pred.dtype != target.dtype:
        raise ValueError(f"image_metrics: pred is {pred.dtype}, target {target.dtype}")
    dt = dtype_id(pred)
    B, H, W, C = pred.shape
    pred, target = pred.contiguous(), target.contiguous()
    if mask is not None:
        require_cuda(mask)
        if mask.dim() == 2:
            mask = mask[None]
        if tuple(mask.shape) != (B, H, W):
            raise ValueError(f"image_metrics: mask must be [B, H, W] = {(B, H, W)}, got {tuple(mask.shape)}")
        mask = mask.to(torch.float32).contiguous()
    dev = pred.device
    with torch.cuda.device(dev):
        need = query_u64(lib.cnerf_image_metrics_workspace_bytes, B, H, W, C)         # ValueError on an unsupported shape, before any allocation
        sums = torch.empty(B, 5, dtype=torch.float64, device=dev)
        ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
        smap = torch.empty(B, H - (WINDOW - 1), W - (WINDOW - 1), C, dtype=torch.float32, device=dev) if want_map else None
        check(lib.cnerf_image_metrics(ptr(pred), ptr(target), ptr(mask), B, H, W, C, dt, int(bool(quantize)), ptr(sums), ptr(smap), ptr(ws),
                                      stream()), "image_metrics")
    se, ae, n, ss, nw = sums.unbind(1)
    mse = se / n                                                                       # 0 / 0 = nan where nothing is counted
    out = {'mse': mse, 'l1': ae / n, 'psnr': 10.0 * torch.log10(1.0 / mse), 'ssim': ss / nw, 'n_pixels': n, 'n_windows': nw}
    if want_map:
        out['ssim_map'] = smap
    return out


def to_uint8(image):
    """floor(clamp(v, 0, 1) * 255) as uint8, in float32: the bytes the trainers' evaluate() / test() write, and the rule behind
    image_metrics(quantize=True) — the reference's `(pred * 255).astype(np.uint8)` (utils_init_nerf.py:550) plus a clamp"""
    return (image.float().clamp(0.0, 1.0) * 255.0).floor().to(torch.uint8)


def psnr(pred, target, mask=None, quantize=False):
    """[B] float64: image_metrics(...)['psnr']"""
    return image_metrics(pred, target, mask, quantize)['psnr']


def ssim(pred, target, mask=None, quantize=False):
    """[B] float64: image_metrics(...)['ssim']"""
    return image_metrics(pred, target, mask, quantize)['ssim']


def _cos(a, b):
    a, b = a.double(), b.double()
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


def clip_scores(clip, source_images, edited_images, source_text, edited_text):
    """The edit scores of the CustomNeRF paper from the CLIP towers of sd.clip_view.CLIP (`clip`): per image, float64 [B],
        'clip_text_image'  = cos(E_img(edited), E_txt(edited_text))
        'clip_directional' = cos(E_img(edited) - E_img(source), E_txt(edited_text) - E_txt(source_text))
    source_images / edited_images: whatever clip.encode_img takes ([B, 3, H, W] in [0, 1]); source_text / edited_text: one prompt each — a
    string or list of one string when `clip` has a tokenizer injected, token ids [1, 77] otherwise, as everywhere else in the package.
    Host-side composition on the [B, D] embeddings the encoders return; no kernel of its own."""
    with torch.no_grad():
        e_src, e_edit = clip.encode_img(source_images), clip.encode_img(edited_images)
        t_src, t_edit = clip.get_text_embeds(source_text), clip.get_text_embeds(edited_text)
    e_src, e_edit, t_src, t_edit = e_src.double(), e_edit.double(), t_src.double(), t_edit.double()
    if t_src.shape[0] != 1 or t_edit.shape[0] != 1:
        raise ValueError("clip_scores: one source prompt and one edited prompt")
    return {'clip_text_image': _cos(e_edit, t_edit), 'clip_directional': _cos(e_edit - e_src, t_edit - t_src)}
