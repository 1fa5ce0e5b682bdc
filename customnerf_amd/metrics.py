"""Image scores on the GPU: PSNR, L1 and SSIM of rendered views (cnerf_image_metrics, csrc/metrics.hip), the differentiable SSIM loss
(ssim_loss / ssim_with_grad, cnerf_ssim_grad), and the CLIP scores of an edit.

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


def _as_batch(t, what, who="image_metrics"):
    if not torch.is_tensor(t):
        raise TypeError(f"{who}: {what} must be a tensor")
    require_cuda(t)
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise ValueError(f"{who}: {what} must be [B, H, W, C] or [H, W, C], got {tuple(t.shape)}")
    return t


def _prepare(pred, target, mask, who):
    """the argument rules image_metrics and the SSIM gradient share -> contiguous pred, target [B, H, W, C], mask float32 [B, H, W] or None, dtype id"""
    pred, target = _as_batch(pred, "pred", who), _as_batch(target, "target", who)
    if pred.shape != target.shape:
        raise ValueError(f"{who}: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if pred.dtype != target.dtype:
        raise ValueError(f"{who}: pred is {pred.dtype}, target {target.dtype}")
    dt = dtype_id(pred)
    B, H, W, C = pred.shape
    pred, target = pred.contiguous(), target.contiguous()
    if mask is not None:
        require_cuda(mask)
        if mask.dim() == 2:
            mask = mask[None]
        if tuple(mask.shape) != (B, H, W):
            raise ValueError(f"{who}: mask must be [B, H, W] = {(B, H, W)}, got {tuple(mask.shape)}")
        mask = mask.to(torch.float32).contiguous()
    return pred, target, mask, dt


def image_metrics(pred, target, mask=None, quantize=False, want_map=False):
    """pred, target: CUDA tensors [B, H, W, C] or [H, W, C], float32 or float16 (both the same), C in {1, 3}, values nominally in [0, 1];
    mask: None or [B, H, W] / [H, W] (any real dtype or bool; nonzero = the pixel counts).  Non-contiguous tensors are made contiguous.
    -> dict of [B] float64 CUDA tensors: 'mse', 'l1', 'psnr' (= 10 log10(1 / mse), inf at mse == 0), 'ssim', 'n_pixels' (counted
    pixel-channels), 'n_windows' (counted window-channels), and with want_map 'ssim_map' [B, H - 10, W - 10, C] float32 (the whole map,
    whatever the mask says).  The module docstring defines SSIM and `quantize`.  Runs on the current stream, no host sync."""
    pred, target, mask, dt = _prepare(pred, target, mask, "image_metrics")
    B, H, W, C = pred.shape
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


def _ssim_grad_call(pred, target, mask, who):
    """one cnerf_ssim_grad call -> (sums [B, 5] float64 as image_metrics forms them, grad_unit [B, H, W, C] float32)"""
    pred, target, mask, dt = _prepare(pred, target, mask, who)
    B, H, W, C = pred.shape
    dev = pred.device
    with torch.cuda.device(dev):
        need = query_u64(lib.cnerf_ssim_grad_workspace_bytes, B, H, W, C)               # ValueError on an unsupported shape, before any allocation
        sums = torch.empty(B, 5, dtype=torch.float64, device=dev)
        grad = torch.empty(B, H, W, C, dtype=torch.float32, device=dev)
        ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
        check(lib.cnerf_ssim_grad(ptr(pred), ptr(target), ptr(mask), B, H, W, C, dt, ptr(sums), ptr(grad), ptr(ws), stream()), who)
    return sums, grad


def ssim_with_grad(pred, target, mask=None):
    """The raw pieces of the SSIM loss, arguments as image_metrics: -> (ssim [B] float64, grad_unit [B, H, W, C] float32), grad_unit =
    d ssim_b / d pred (include/customnerf_hip.h cnerf_ssim_grad has the formulas): float64 throughout, rounded to float32 once, bit-reproducible.
    An image with no counted window has ssim nan (as image_metrics reports it) and a gradient of exact zeros.  Nothing here is recorded by
    autograd; no host sync."""
    with torch.no_grad():
        sums, grad = _ssim_grad_call(pred, target, mask, "ssim_with_grad")
        return sums[:, 3] / sums[:, 4], grad


class _SsimLoss(torch.autograd.Function):
    """[B] float32 1 - ssim_b (0 where no window counts); the gradient comes out of the forward's one cnerf_ssim_grad call (as _ReconLoss does)"""

    @staticmethod
    def forward(ctx, pred, target, mask):
        sums, grad = _ssim_grad_call(pred, target, mask, "ssim_loss")
        counted = sums[:, 4] > 0
        loss = torch.where(counted, 1.0 - sums[:, 3] / sums[:, 4], torch.zeros_like(sums[:, 3])).to(torch.float32)
        ctx.save_for_backward(grad)
        ctx.like = (pred.dtype, tuple(pred.shape))
        ctx.mark_non_differentiable(counted)
        return loss, counted

    @staticmethod
    def backward(ctx, g_loss, _g_counted):
        grad, = ctx.saved_tensors
        dtype, shape = ctx.like
        g = (grad * (-g_loss.to(torch.float32)).reshape(-1, 1, 1, 1)).to(dtype)          # the product in float32, one rounding to pred's dtype
        return g.reshape(shape), None, None


def ssim_loss(pred, target, mask=None, reduction='mean'):
    """The D-SSIM term of a training loss: float32 1 - ssim_b, SSIM as the module docstring defines it (what image_metrics scores, unquantized).
    pred, target: [B, H, W, C] or [H, W, C], float32 or float16 (both the same), C in {1, 3}; mask as in image_metrics (a window counts when its
    centre pixel does).  reduction 'none' -> [B], 0 for an image with no counted window; 'mean' -> the mean over the images that have one, 0 if
    none has.  Differentiable in pred only: target and mask get NO gradient (a target that requires grad keeps grad None).  The backward
    multiplies the gradient stored by the forward pass in float32 and casts to pred.dtype once, so a loss scaler's factor is applied before any
    half rounding.  One cnerf_ssim_grad call in the forward pass, no host sync: it can be captured in a graph."""
    if reduction not in ('mean', 'none'):
        raise ValueError(f"ssim_loss: reduction must be 'mean' or 'none', got {reduction!r}")
    if torch.is_tensor(target):
        target = target.detach()
    loss, counted = _SsimLoss.apply(pred, target, mask)
    if reduction == 'none':
        return loss
    return loss.sum() / counted.sum().clamp(min=1).to(torch.float32)


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
