"""CPU: what the evaluation feature promises without a GPU.
  * tests/ssim_restatement.py, the float64 NumPy reference the GPU tests of tests/test_gpu_metrics.py compare against, checked on cases
    whose answer is known in closed form;
  * cnerf_image_metrics / _workspace_bytes decide their return codes before any launch;
  * inter_pose_num against the reference's own function (tests/golden/inter_pose.npz, recorded by tests/golden/make_eval_golden.py);
  * the 'test' split's 73-pose trajectory, built without a device;
  * mesh.write_apng read back with PIL.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ssim_restatement as R  # noqa: E402


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_identical_images_are_exactly_one():
    x = np.random.default_rng(0).random((2, 19, 23, 3)).astype(np.float32)
    m = R.metrics(x, x)
    assert np.all(m["ssim_map"] == 1.0) and m["ssim_map"].shape == (2, 9, 13, 3)
    assert np.all(m["ssim"] == 1.0) and np.all(np.isposinf(m["psnr"])) and np.all(m["mse"] == 0.0)
    assert np.all(m["n_pixels"] == 19 * 23 * 3) and np.all(m["n_windows"] == 9 * 13 * 3)


@pytest.mark.parametrize("a, b", [(1.0, 0.9), (0.25, 0.75), (0.0, 1.0), (0.5, 0.5)])
def test_restatement_constant_images_closed_form(a, b):
    """flat images: both variances and the covariance vanish, ssim = (2ab + C1) / (a^2 + b^2 + C1)"""
    x, y = np.full((1, 15, 17, 1), a, np.float32), np.full((1, 15, 17, 1), b, np.float32)
    a, b = float(np.float32(a)), float(np.float32(b))
    want = (2 * a * b + 1e-4) / (a * a + b * b + 1e-4)
    m = R.metrics(x, y)
    assert np.abs(m["ssim_map"] - want).max() <= 1e-12 and abs(m["ssim"][0] - want) <= 1e-12
    assert abs(m["mse"][0] - (a - b) ** 2) <= 1e-15 and abs(m["l1"][0] - abs(a - b)) <= 1e-15


def test_restatement_window_masks_and_quantize():
    rng = np.random.default_rng(1)
    x, y = rng.random((1, 11, 11, 3)).astype(np.float32), rng.random((1, 11, 11, 3)).astype(np.float32)
    m = R.metrics(x, y)
    assert m["ssim_map"].shape == (1, 1, 1, 3) and m["n_windows"][0] == 3                   # H = W = 11: exactly one window per channel
    g = R.window()
    assert g.shape == (11,) and abs(g.sum() - 1.0) <= 1e-15 and np.all(g == g[::-1]) and abs(g[5] / g[4] - np.exp(1 / 4.5)) <= 1e-15
    w2 = np.outer(g, g)                                                                     # the one window, formed directly
    for c in range(3):
        a, b = x[0, :, :, c].astype(np.float64), y[0, :, :, c].astype(np.float64)
        mu_a, mu_b = (w2 * a).sum(), (w2 * b).sum()
        va, vb, cov = (w2 * a * a).sum() - mu_a ** 2, (w2 * b * b).sum() - mu_b ** 2, (w2 * a * b).sum() - mu_a * mu_b
        want = (2 * mu_a * mu_b + 1e-4) * (2 * cov + 9e-4) / ((mu_a ** 2 + mu_b ** 2 + 1e-4) * (va + vb + 9e-4))
        assert abs(m["ssim_map"][0, 0, 0, c] - want) <= 1e-12
    # masks: the centre pixel decides the window; an empty mask is nan with a count of 0
    mask = np.zeros((1, 11, 11), np.float32)
    e = R.metrics(x, y, mask)
    assert e["n_pixels"][0] == 0 and e["n_windows"][0] == 0 and np.isnan(e["ssim"][0]) and np.isnan(e["mse"][0]) and np.isnan(e["psnr"][0])
    mask[0, 5, 5] = 2.0
    one = R.metrics(x, y, mask)
    assert one["n_pixels"][0] == 3 and one["n_windows"][0] == 3 and abs(one["ssim"][0] - m["ssim"][0]) <= 1e-15
    assert abs(one["mse"][0] - ((x[0, 5, 5].astype(np.float64) - y[0, 5, 5]) ** 2).mean()) <= 1e-15
    mask[:] = 0
    mask[0, 0, 0] = 1.0
    off = R.metrics(x, y, mask)
    assert off["n_pixels"][0] == 3 and off["n_windows"][0] == 0 and np.isnan(off["ssim"][0])
    # quantize truncates: 0.999 -> 254 / 255, it does not round to 1; and clamps
    q = R.quantize(np.array([0.999, 1.0, 1.7, -0.2, 0.5, 254.5 / 255], np.float32))
    np.testing.assert_array_equal(q, (np.array([254, 255, 255, 0, 127, 254], np.float32) / np.float32(255)))
    mq = R.metrics(x, y, quantize_images=True)
    md = R.metrics(R.quantize(x), R.quantize(y))
    assert mq["mse"][0] == md["mse"][0] and mq["ssim"][0] == md["ssim"][0] and mq["mse"][0] != m["mse"][0]


# ------------------------------------------------------------------------------------------------ argument validation without a launch
def test_image_metrics_argument_validation_without_launch():
    from customnerf_amd._lib import lib
    one = ctypes.c_void_p(16)                  # non-NULL, 8-byte aligned dummy, never dereferenced on these paths
    need = ctypes.c_uint64(0)

    def ws(B, H, W, C):
        need.value = 123
        rc = lib.cnerf_image_metrics_workspace_bytes(B, H, W, C, ctypes.addressof(need))
        return rc, need.value

    def call(pred=one, target=one, mask=None, B=1, H=16, W=16, C=3, dtype=0, quantize=0, sums=one, smap=None, work=one):
        return lib.cnerf_image_metrics(pred, target, mask, B, H, W, C, dtype, quantize, sums, smap, work, None)

    assert call(H=10) == -1 and call(W=10) == -1 and call(H=10, W=10) == -1                 # below one window: refused
    assert call(C=2) == -1 and call(C=0) == -1 and call(C=4) == -1
    assert call(dtype=7) == -1
    assert call(pred=None) == -2 and call(target=None) == -2 and call(sums=None) == -2 and call(work=None) == -2
    assert call(work=ctypes.c_void_p(20)) == -1                                             # float64 partials: 8-byte alignment
    assert call(B=0, pred=None, sums=None) == 0                                             # empty work is accepted without a launch
    assert ws(1, 10, 16, 3)[0] == -1 and ws(1, 16, 10, 3)[0] == -1 and ws(1, 16, 16, 2)[0] == -1
    assert lib.cnerf_image_metrics_workspace_bytes(1, 16, 16, 3, None) == -2
    # five float64 sums per 32 x 32 tile of the valid region, per image and channel
    assert ws(1, 11, 11, 1) == (0, 40) and ws(1, 42, 42, 1) == (0, 40) and ws(1, 43, 42, 1) == (0, 80) and ws(2, 43, 43, 3) == (0, 2 * 3 * 4 * 40)
    prev = 0
    for n in (1, 2, 3, 8):
        cur = ws(n, 100, 100, 3)[1]
        assert cur > prev
        prev = cur
    for axis in (0, 1):
        prev = 0
        for e in (11, 12, 42, 43, 74, 75, 800, 4000):
            cur = ws(1, *((e, 64) if axis == 0 else (64, e)), 3)[1]
            assert cur >= prev and cur > 0                                                  # monotone in H and in W
            prev = cur
        assert prev > ws(1, 64, 64, 3)[1]


def test_image_metrics_python_validation():
    from customnerf_amd import metrics as M
    x = torch.zeros(1, 16, 16, 3)
    with pytest.raises(RuntimeError):
        M.image_metrics(x, x)                                                               # CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError):
        M.psnr(x[0], x[0])
    u = M.to_uint8(torch.tensor([0.999, 1.0, 1.7, -0.2, 0.5]))
    assert u.dtype == torch.uint8 and u.tolist() == [254, 255, 255, 0, 127]


# ------------------------------------------------------------------------------------------------ pose interpolation
CASES = ("general", "same_rot", "turn179", "scaled")


@pytest.mark.parametrize("case", CASES)
def test_inter_pose_num_matches_reference_golden(golden, case):
    """1e-6 absolute: the reference inverts in float32 and returns float32; entries are at most ~2 in magnitude (rotation entries <= 1,
    |translation| <= 1 times a scale <= 2), so a float32 rounding is <= 1.2e-7 and the three float32 inversions on its path a small
    multiple of that.  (This implementation works in float64 and rounds once.)"""
    from customnerf_amd.nerf.provider import inter_pose_num
    g = golden("inter_pose")
    p0, p1, scale, want = (g[f"{case}__{k}"] for k in ("pose_0", "pose_1", "scale", "poses"))
    got = inter_pose_num(torch.from_numpy(p0), torch.from_numpy(p1), len(want), scale=scale)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (7, 4, 4)
    err = np.abs(got.numpy().astype(np.float64) - want).max()
    print(f"inter_pose_num[{case}]: max |diff| to the reference {err:.3e}")
    assert err <= 1e-6


def test_inter_pose_endpoints_and_no_scipy(golden):
    from customnerf_amd.nerf.provider import inter_pose, inter_pose_num
    g = golden("inter_pose")
    for case in CASES[:3]:                                                                  # scale 1: ratio 0 and 1 give the poses back
        p0, p1 = g[f"{case}__pose_0"], g[f"{case}__pose_1"]
        for ratio, want in ((0.0, p0), (1.0, p1)):
            got = inter_pose(torch.from_numpy(p0), torch.from_numpy(p1), ratio, 1.0)
            assert got.dtype == np.float32 and got.shape == (4, 4)
            assert np.abs(got - want).max() <= 2 * np.finfo(np.float32).eps * max(1.0, np.abs(want).max())
    assert inter_pose_num(torch.eye(4), torch.eye(4)).shape == (120, 4, 4)                  # the reference's default count
    # rotations stay rotations along the way, the 179-degree turn included
    mid = inter_pose_num(torch.from_numpy(g["turn179__pose_0"]), torch.from_numpy(g["turn179__pose_1"]), 9)[:, :3, :3].double()
    assert (mid @ mid.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-6
    import inspect
    import re
    from customnerf_amd.nerf import provider
    assert not re.search(r"^\s*(import|from)\s+scipy", inspect.getsource(provider), flags=re.M)  # a slerp of its own


def _ring(V):
    poses = []
    for i in range(V):
        th = 2 * np.pi * i / V
        eye = np.array([np.cos(th), np.sin(th), 0.3])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0, 0, 1.0])
        right /= np.linalg.norm(right)
        m = np.zeros((3, 4))
        m[:, 0], m[:, 1], m[:, 2], m[:, 3] = right, np.cross(right, fwd), -fwd, eye
        poses.append(m)
    return torch.from_numpy(np.stack(poses).astype(np.float32))


def test_test_trajectory_pose_list():
    from customnerf_amd.nerf.provider import inter_pose_num, key_view_indices, trajectory_poses
    c2w = _ring(9)
    assert key_view_indices(9).tolist() == [0, 2, 5, 8] and key_view_indices(8).tolist() == [0, 2, 4, 7]
    traj = trajectory_poses(c2w)
    assert traj.dtype == torch.float32 and tuple(traj.shape) == (73, 3, 4)                  # 3 legs of 25, shared endpoints once
    fwd = traj.flip(0)                                                                      # the list is reversed: undo it
    keys = c2w[[0, 2, 5, 8]]
    for j, k in enumerate((0, 24, 48, 72)):
        assert (fwd[k] - keys[j]).abs().max() <= 1e-6
    full = lambda m: torch.cat([m, torch.tensor([[0.0, 0.0, 0.0, 1.0]])], dim=0)
    for leg in range(3):
        want = inter_pose_num(full(keys[leg]), full(keys[leg + 1]), 25, scale=np.ones(3))[:, :3]
        first = 0 if leg == 0 else 1                                                        # a shared endpoint is the EARLIER leg's last pose
        assert torch.equal(fwd[24 * leg + first:24 * leg + 25], want[first:])
    d = (fwd[1:] - fwd[:-1]).abs().amax(dim=(1, 2))
    assert float(d.min()) > 1e-4                                                            # no pose twice: the shared endpoints were dropped
    # dis_scale reaches the interpolation, per component
    s = trajectory_poses(c2w, dis_scale=(0.5, 1.0, 2.0))
    assert tuple(s.shape) == (73, 3, 4) and not torch.equal(s, traj)
    assert torch.equal(s.flip(0)[:25], inter_pose_num(full(keys[0]), full(keys[1]), 25, scale=np.array([0.5, 1.0, 2.0]))[:, :3])


# ------------------------------------------------------------------------------------------------ APNG
def _frames(n, H=5, W=7, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("n, fps", [(3, 30), (1, 10), (6, 7)])
def test_write_apng_reads_back(tmp_path, n, fps):
    from PIL import Image
    from customnerf_amd.mesh import write_apng
    fr = _frames(n)
    path = str(tmp_path / "a.png")
    write_apng(path, [torch.from_numpy(f) for f in fr] if n == 3 else fr, fps=fps, loop=2)
    im = Image.open(path)
    assert im.format == "PNG" and im.size == (7, 5) and getattr(im, "n_frames", 1) == n
    for i in range(n):
        im.seek(i)
        np.testing.assert_array_equal(np.asarray(im.convert("RGB")), fr[i])
        if n > 1:
            assert abs(im.info["duration"] - 1000.0 / fps) <= 1e-6 and im.info["loop"] == 2
    # chunk order and the running sequence numbers, straight from the bytes
    import struct
    raw, pos, tags, seqs = open(path, "rb").read(), 8, [], []
    while pos < len(raw):
        (ln,), tag = struct.unpack(">I", raw[pos:pos + 4]), raw[pos + 4:pos + 8]
        tags.append(tag)
        if tag in (b"fcTL", b"fdAT"):
            seqs.append(struct.unpack(">I", raw[pos + 8:pos + 12])[0])
        pos += 12 + ln
    assert tags == [b"IHDR", b"acTL", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (n - 1) + [b"IEND"]
    assert seqs == list(range(2 * n - 1))


def test_write_apng_rejects_bad_frames(tmp_path):
    from customnerf_amd.mesh import write_apng
    fr = _frames(2)
    path = str(tmp_path / "b.png")
    with pytest.raises(ValueError):
        write_apng(path, [fr[0], np.zeros((5, 8, 3), np.uint8)])                            # another size
    with pytest.raises(ValueError):
        write_apng(path, [fr[0], fr[1].astype(np.float32) / 255])                           # not uint8
    with pytest.raises(ValueError):
        write_apng(path, [torch.zeros(5, 7, 3)])
    with pytest.raises(ValueError):
        write_apng(path, [])
    with pytest.raises(ValueError):
        write_apng(path, [fr[0][:, :, :1]])
    with pytest.raises(ValueError):
        write_apng(path, fr, fps=0)
    assert not os.path.exists(path)
