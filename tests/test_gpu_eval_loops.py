"""GPU: the 'val' / 'test' splits of NerfstudioScene and the trainers' evaluate() / test() loops on a small scene on disk (8 views, 24 x 24 after
the area resize).  Nothing is trained to a quality threshold: the loops are checked for equality with what they are built from — eval_step's
own panels, test_step's own output, torch float64 arithmetic on them — not for a PSNR that would depend on the machine."""
import copy
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

V, H, W = 8, 24, 24


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    from test_provider import _write_scene
    root = str(tmp_path_factory.mktemp("eval_scene"))
    _write_scene(root, V=V, H=H, W=W)
    return root


@pytest.fixture(scope="module")
def recon(scene_dir):
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)
    torch.manual_seed(0)
    opt = sc.make_opt(fp16=True, num_levels=8, num_steps=16, upsample_steps=16, iters=200)
    model = NeRFNetwork(opt).cuda()
    with torch.no_grad():
        model.pos_en.embeddings.uniform_(-0.5, 0.5)                                          # renders that are not one flat colour
    return ReconTrainer(model, opt, fp16=True)


def test_splits(scene_dir):
    from customnerf_amd.nerf.provider import NerfstudioScene, trajectory_poses
    plain = NerfstudioScene(scene_dir, resolution_level=2, device="cuda")
    train = NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='train')
    assert len(plain) == len(train) == V and (train.H, train.W) == (H, W)
    for a, b in ((plain.rays_o, train.rays_o), (plain.rays_d, train.rays_d), (plain.images, train.images), (plain.masks, train.masks)):
        assert torch.equal(a, b)                                                             # 'train' is what it was, bit for bit
    assert plain.image_paths == train.image_paths and torch.equal(plain.camera_to_world, train.camera_to_world)
    val = NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='val')
    keep = [0, 2, 4, 7]
    assert len(val) == 4 and val.image_paths == [train.image_paths[i] for i in keep]
    assert torch.equal(val.images, train.images[keep]) and torch.equal(val.masks, train.masks[keep])
    assert torch.equal(val.rays_o, train.rays_o[keep]) and torch.equal(val.rays_d, train.rays_d[keep])
    rgbs, mask, ro, rd, h, w, path = val[3]
    assert rgbs.shape == (1, H * W, 3) and mask.shape == (1, H * W) and ro.shape == (1, H * W, 3) and (h, w) == (H, W) and path == train.image_paths[7]
    assert len(NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='val', val_all_images=True)) == V
    test = NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='test', dis_scale=(1, 1, 1))
    assert len(test) == 73 and test.images is None and test.masks is None
    assert torch.equal(test.camera_to_world, trajectory_poses(train.camera_to_world))
    for i in (0, 36, 72):
        rgbs, mask, ro, rd, h, w, _ = test[i]
        assert rgbs is None and mask is None and ro.shape == (1, H * W, 3) and rd.shape == (1, H * W, 3) and (h, w) == (H, W)
    # the reversed list: the trajectory ends at key view 0 and starts at key view 7 (same rays, to the rounding of the pose round trip)
    assert float((test.rays_o[72] - train.rays_o[0]).abs().max()) <= 1e-5 and float((test.rays_d[0] - train.rays_d[7]).abs().max()) <= 1e-5
    scaled = NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='test', dis_scale=(0.5, 1, 2))
    assert len(scaled) == 73 and not torch.equal(scaled.rays_o, test.rays_o)
    same = NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='test', dont_inter_test=True)
    assert len(same) == V and torch.equal(same.rays_d, train.rays_d)
    with pytest.raises(ValueError):
        NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='dev')


def test_evaluate(scene_dir, recon, tmp_path):
    from customnerf_amd.nerf.provider import NerfstudioScene
    val = NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='val')
    recon.model.train()
    out = recon.evaluate(val, save_path=str(tmp_path), name="ep0")
    assert recon.model.training                                                              # the mode it was in is restored
    assert len(out['views']) == 4 and set(out['mean']) == set(out['views'][0])
    recon.model.eval()
    for i, row in enumerate(out['views']):
        panel = recon.eval_step(val[i])[0]
        assert panel.shape == (1, H, 7 * W, 3)
        gt, pred = panel[:, :, :W].double(), panel[:, :, W:2 * W].double()
        mse = float(((pred - gt) ** 2).mean())
        assert abs(row['psnr'] - 10 * math.log10(1 / mse)) <= 1e-10 * abs(row['psnr']) and abs(row['mse'] - mse) <= 1e-10 * mse
        assert abs(row['l1'] - float((pred - gt).abs().mean())) <= 1e-10 * row['l1']
        m = val[i][1].reshape(1, H, W) != 0
        assert row['fg_n_pixels'] == float(m.sum()) * 3 and row['fg_n_pixels'] + row['bg_n_pixels'] == H * W * 3
        if m.any():
            fg_mse = float(((pred - gt) ** 2)[m].mean())
            assert abs(row['fg_mse'] - fg_mse) <= 1e-10 * fg_mse
        else:
            assert math.isnan(row['fg_mse']) and math.isnan(row['fg_ssim']) and abs(row['bg_mse'] - mse) <= 1e-10 * mse
        assert -1.0 <= row['ssim'] <= 1.0
        gt_m, pr_m = panel[0, :, 3 * W:4 * W, 0] > 0.5, panel[0, :, 4 * W:5 * W, 0] > 0.5
        union = float((gt_m | pr_m).sum())
        if union:
            assert abs(row['mask_iou'] - float((gt_m & pr_m).sum()) / union) <= 1e-12
        else:
            assert math.isnan(row['mask_iou'])
    recon.model.train()
    assert any(r['fg_n_pixels'] > 0 for r in out['views']) and any(r['fg_n_pixels'] == 0 for r in out['views'])   # masks exist for every second frame
    finite = [r['psnr'] for r in out['views']]
    assert abs(out['mean']['psnr'] - sum(finite) / 4) <= 1e-12 * abs(out['mean']['psnr'])
    # files: four panels and the scores
    from PIL import Image
    for i in range(4):
        im = np.asarray(Image.open(os.path.join(str(tmp_path), "ep0", f"{i:04d}.png")).convert("RGB"))
        assert im.shape == (H, 7 * W, 3)
    loaded = json.load(open(os.path.join(str(tmp_path), "ep0", "metrics.json")))
    assert len(loaded['views']) == 4 and loaded['views'][0]['psnr'] == out['views'][0]['psnr'] and set(loaded['mean']) == set(out['mean'])
    # quantize=True scores what the written panels hold
    q = recon.evaluate(val, quantize=True)
    gt8, pred8 = (np.float32(im[:, :W]) / np.float32(255)).astype(np.float64), (np.float32(im[:, W:2 * W]) / np.float32(255)).astype(np.float64)
    mse8 = float(((pred8 - gt8) ** 2).mean())
    assert abs(q['views'][3]['mse'] - mse8) <= 1e-10 * mse8
    test_views = NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='test')
    with pytest.raises(ValueError):
        recon.evaluate(test_views)                                                           # no images to compare with


def test_edit_trainer_evaluate_against(scene_dir, recon):
    from customnerf_amd import scene as sc
    from customnerf_amd.nerf.provider import NerfstudioScene
    from customnerf_amd.sd import arch
    from customnerf_amd.sd.editing import EditTrainer
    from customnerf_amd.sd.guidance import StableDiffusion
    opt = sc.make_opt(fp16=True, num_levels=8, num_steps=16, upsample_steps=16, cfg=7.5, log_loss_item=False, keep_bg=10.0, lambda_sd=0.01)
    model = copy.deepcopy(recon.model)
    pre = copy.deepcopy(model).eval()
    guide = StableDiffusion("cuda", "1.5", opt, unet_state=arch.random_state_dict(arch.unet_params(arch.UNET_TINY), 1),
                            vae_state=arch.random_state_dict(arch.vae_encoder_params(arch.VAE_TINY), 2), unet_cfg=arch.UNET_TINY, vae_cfg=arch.VAE_TINY)
    tr = EditTrainer(model, pre, guide, opt, guide.synthetic_text_embeds(0), guide.synthetic_text_embeds(1))
    val = NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='val')
    same = tr.evaluate(val, against=tr.model)                                                # a field against itself: nothing changed anywhere
    for row in same['views']:
        assert row['psnr'] == math.inf and row['ssim'] == 1.0 and row['bg_psnr'] == math.inf and row['bg_ssim'] == 1.0 and row['bg_mse'] == 0.0
        assert row['fg_n_pixels'] + row['bg_n_pixels'] == H * W * 3
        assert 'mask_iou' not in row
    assert same['mean']['bg_psnr'] == math.inf and same['mean']['bg_ssim'] == 1.0
    # against the pretrained copy after the edited field moved: the report is the masked score between the two renders
    with torch.no_grad():
        model.pos_en.embeddings.mul_(0.5)
    rep = tr.evaluate(val, against=tr.model_pretrained)
    tr.model.eval()
    rgbs, mask, ro, rd, h, w, _ = val[0]
    a = tr._render_eval(pre, ro, rd)['image'].reshape(1, H, W, 3).double()
    b = tr._render_eval(tr.model, ro, rd)['image'].reshape(1, H, W, 3).double()
    bg = mask.reshape(1, H, W) == 0
    want = float(((a - b) ** 2)[bg].mean())
    assert want > 0 and abs(rep['views'][0]['bg_mse'] - want) <= 1e-10 * want and rep['views'][0]['bg_psnr'] < math.inf


def test_test_loop_writes_frames_and_apng(scene_dir, recon, tmp_path):
    from PIL import Image
    from customnerf_amd.nerf.provider import NerfstudioScene
    traj = NerfstudioScene(scene_dir, resolution_level=2, device="cuda", split='test')
    views = [traj[i] for i in (0, 36, 72)]
    recon.model.train()
    out = recon.test(views, str(tmp_path), name="walk", fps=12)
    assert recon.model.training
    assert [os.path.basename(p) for p in out['frames']] == ["000.png", "001.png", "002.png"] and all(os.path.dirname(p) == os.path.join(str(tmp_path), "walk") for p in out['frames'])
    assert out['video'] == os.path.join(str(tmp_path), "walk_rgb.png")
    assert sorted(os.listdir(str(tmp_path))) == ["walk", "walk_rgb.png"] and len(os.listdir(os.path.join(str(tmp_path), "walk"))) == 3
    recon.model.eval()
    anim = Image.open(out['video'])
    assert anim.n_frames == 3 and abs(anim.info["duration"] - 1000.0 / 12) <= 1e-6
    for i, v in enumerate(views):
        pred = recon.test_step(v)[0][0]
        want = (pred.clamp(0, 1) * 255).floor().to(torch.uint8).cpu().numpy()                # the quantize rule on test_step's own output
        np.testing.assert_array_equal(np.asarray(Image.open(out['frames'][i]).convert("RGB")), want)
        anim.seek(i)
        np.testing.assert_array_equal(np.asarray(anim.convert("RGB")), want)
    recon.model.train()
    still = recon.test(views[:1], str(tmp_path / "novideo"), write_video=False)
    assert still['video'] is None and len(still['frames']) == 1 and os.listdir(str(tmp_path / "novideo")) == ["test"]
