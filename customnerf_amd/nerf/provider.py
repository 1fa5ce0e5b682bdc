"""Dataset front-end for nerfstudio-format scenes: counterpart of NerfstudioData._load_renderings /
get_focal_lengths / _generate_rays (nerf/provider.py:201-470) + auto_orient_and_center_poses (nerf/provider_utils.py:35-115),
feeding the ray kernel (cnerf_generate_rays).  Host-side plumbing: JSON, PIL decoding and a handful of 4x4 matrices on the CPU;
rays, images and masks end up resident on the GPU, one entry per training view.

Differences from the reference, by design: images are area-resized with PIL's BOX filter (cv2 is not a dependency; identical to
cv2.INTER_AREA for integer `resolution_level`), everything stays on the device (the reference keeps numpy lists and re-uploads),
the OPENCV_FISHEYE undistortion branch is not built (pinhole only; raises)."""
import json
import math
import os

import numpy as np
import torch


def rotation_matrix(a, b):
    """provider_utils.py:35-57: rotation taking direction a to direction b (Rodrigues)."""
    a = a / torch.linalg.norm(a)
    b = b / torch.linalg.norm(b)
    v = torch.linalg.cross(a, b)
    c = torch.dot(a, b)
    if c < -1 + 1e-8:                                           # exactly opposite: perturb (the reference draws torch.rand here)
        eps = (torch.rand(3) - 0.5) * 0.01
        return rotation_matrix(a + eps, b)
    s = torch.linalg.norm(v)
    k = torch.tensor([[0.0, -float(v[2]), float(v[1])], [float(v[2]), 0.0, -float(v[0])], [-float(v[1]), float(v[0]), 0.0]])
    return torch.eye(3) + k + k @ k * ((1 - c) / (s ** 2 + 1e-8))


def auto_orient_and_center_poses(poses, method="up", center_poses=True):
    """provider_utils.py:60-115 ("up" and "none"; "pca" is never used by the reference's loader).  poses [V,4,4] ->
    (oriented [V,3,4], transform [3,4])."""
    poses = torch.as_tensor(poses, dtype=torch.float32)
    translation = poses[..., :3, 3]
    mean_translation = torch.mean(translation, dim=0)
    translation = mean_translation if center_poses else torch.zeros_like(mean_translation)
    if method == "up":
        up = torch.mean(poses[:, :3, 1], dim=0)
        up = up / torch.linalg.norm(up)
        rotation = rotation_matrix(up, torch.tensor([0.0, 0.0, 1.0]))
        transform = torch.cat([rotation, rotation @ -translation[..., None]], dim=-1)
    elif method == "none":
        transform = torch.eye(4)
        transform[:3, 3] = -translation
        transform = transform[:3, :]
    else:
        raise ValueError(f"unsupported orientation method {method!r}")
    return transform @ poses, transform


def focal_lengths(meta):
    """provider.py:296-322"""
    def f(rad, res):
        return 0.5 * res / np.tan(0.5 * rad)
    fl_x = meta["fl_x"] if "fl_x" in meta else f(np.deg2rad(meta["x_fov"]), meta["w"]) if "x_fov" in meta else \
        f(meta["camera_angle_x"], meta["w"]) if "camera_angle_x" in meta else 0
    fl_y = meta["fl_y"] if "fl_y" in meta else f(np.deg2rad(meta["y_fov"]), meta["h"]) if "y_fov" in meta else \
        f(meta["camera_angle_y"], meta["h"]) if "camera_angle_y" in meta else 0
    if fl_x == 0 or fl_y == 0:
        raise AttributeError("Focal length cannot be calculated from transforms.json (missing fields).")
    return float(fl_x), float(fl_y)


def _load_image(path, level, mode):
    from PIL import Image
    img = Image.open(path).convert(mode)
    if level != 1:
        img = img.resize((int(img.width / level), int(img.height / level)), Image.BOX)
    return np.asarray(img, dtype=np.float32) / 256.0          # the reference divides by 256 (provider.py:268)


def _quat_from_matrix(m):
    """unit quaternion (w, x, y, z) of a 3x3 rotation, float64 (Shepperd: the largest of the four candidates is the pivot)"""
    t = np.array([m[0, 0] + m[1, 1] + m[2, 2], m[0, 0] - m[1, 1] - m[2, 2], m[1, 1] - m[0, 0] - m[2, 2], m[2, 2] - m[0, 0] - m[1, 1]])
    i = int(np.argmax(t))
    r = math.sqrt(max(1.0 + t[i], 0.0)) * 2.0
    if i == 0:
        q = (0.25 * r, (m[2, 1] - m[1, 2]) / r, (m[0, 2] - m[2, 0]) / r, (m[1, 0] - m[0, 1]) / r)
    elif i == 1:
        q = ((m[2, 1] - m[1, 2]) / r, 0.25 * r, (m[0, 1] + m[1, 0]) / r, (m[0, 2] + m[2, 0]) / r)
    elif i == 2:
        q = ((m[0, 2] - m[2, 0]) / r, (m[0, 1] + m[1, 0]) / r, 0.25 * r, (m[1, 2] + m[2, 1]) / r)
    else:
        q = ((m[1, 0] - m[0, 1]) / r, (m[0, 2] + m[2, 0]) / r, (m[1, 2] + m[2, 1]) / r, 0.25 * r)
    q = np.array(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def _matrix_from_quat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def _slerp(q0, q1, ratio):
    """the rotation `ratio` of the way from q0 to q1 along the shorter arc (what scipy's Slerp, which the reference calls, gives)"""
    d = float(np.dot(q0, q1))
    if d < 0.0:
        q1, d = -q1, -d
    s = float(np.linalg.norm(q1 - d * q0))                          # sin of the angle between the quaternions
    if s < 1e-12:
        return q0                                                    # the same rotation
    th = math.atan2(s, d)
    q = (math.sin((1.0 - ratio) * th) * q0 + math.sin(ratio * th) * q1) / s
    return q / np.linalg.norm(q)


def inter_pose(pose_0, pose_1, ratio, scale):
    """provider.py:31-52: a camera-to-world pose between two, interpolated on the INVERTED (world-to-camera) poses — rotations by slerp,
    translations by lerp times `scale` (a number or three) — and inverted back.  [4, 4] tensors or arrays in; float64 arithmetic with a
    quaternion slerp of its own (the reference goes through scipy and float32 inverses); -> [4, 4] float32 array."""
    p0 = np.linalg.inv(np.asarray(torch.as_tensor(pose_0).detach().cpu().numpy(), dtype=np.float64))
    p1 = np.linalg.inv(np.asarray(torch.as_tensor(pose_1).detach().cpu().numpy(), dtype=np.float64))
    ratio = float(ratio)
    pose = np.eye(4, dtype=np.float64)
    pose[:3, :3] = _matrix_from_quat(_slerp(_quat_from_matrix(p0[:3, :3]), _quat_from_matrix(p1[:3, :3]), ratio))
    pose[:3, 3] = np.asarray(scale, dtype=np.float64) * ((1.0 - ratio) * p0 + ratio * p1)[:3, 3]
    return np.linalg.inv(pose).astype(np.float32)


def inter_pose_num(pose_0, pose_1, num=120, scale=1):
    """provider.py:54-60: `num` poses at ratios linspace(0, 1, num), both ends included -> [num, 4, 4] float32 tensor"""
    return torch.from_numpy(np.stack([inter_pose(pose_0, pose_1, r, scale) for r in np.linspace(0, 1, num)], axis=0))


def key_view_indices(n, count=4):
    """the reference's key views, of the 'val' split and of the 'test' trajectory: linspace(0, n - 1, 4).long() (provider.py:372, :391)"""
    return torch.linspace(0, n - 1, count).to(torch.long)


def trajectory_poses(camera_to_world, dis_scale=(1, 1, 1), per_leg=25):
    """provider.py:370-387, the 'test' split's camera path: between each consecutive pair of the 4 key views `per_leg` interpolated poses
    (inter_pose_num), the endpoint two legs share kept once, and the whole list reversed: 3 * 25 - 2 = 73 poses.  camera_to_world
    [V, 3, 4] (host) -> [73, 3, 4] float32.  Needs no device."""
    c2w = torch.as_tensor(camera_to_world, dtype=torch.float32).cpu()
    keys = c2w[key_view_indices(len(c2w))]
    out = []
    for i in range(len(keys) - 1):
        a, b = torch.eye(4), torch.eye(4)
        a[:3, :4], b[:3, :4] = keys[i], keys[i + 1]
        leg = inter_pose_num(a, b, per_leg, scale=np.asarray(dis_scale, dtype=np.float64))[:, :3, :4]
        out.extend(leg if i == 0 else leg[1:])
    return torch.stack(out[::-1], dim=0).contiguous()


class NerfstudioScene:
    """One nerfstudio-format scene resident on the GPU.  scene[i] -> (rgbs [1,N,3], mask [1,N], rays_o [1,N,3], rays_d [1,N,3], H, W,
    img_path): the tuple the reconstruction / editing steps take (utils_init_nerf.py:195, 354).

    split (provider.py:370-399): 'train' = every training view; 'val' = the 4 views at linspace(0, n - 1, 4).long() with their images and
    masks (all of them with val_all_images); 'test' = the 73-pose trajectory of trajectory_poses(dis_scale) between those 4 views — poses
    only: scene[i] gives None for rgbs and mask and '' for the path, whatever load_images says — or, with dont_inter_test, the training
    views unchanged."""

    def __init__(self, data_dir, keyword="masks", resolution_level=1, device="cuda", train_fraction=0.9, load_images=True, split='train',
                 dis_scale=(1, 1, 1), dont_inter_test=False, val_all_images=False):
        if split not in ('train', 'val', 'test'):
            raise ValueError(f"NerfstudioScene: split must be 'train', 'val' or 'test', got {split!r}")
        from .provider_utils import generate_rays
        self.data_dir, self.level = data_dir, resolution_level
        jf = os.path.join(data_dir, "transforms.json")
        if not os.path.exists(jf):
            jf = os.path.join(data_dir, "transforms_train.json")
        with open(jf, encoding="UTF-8") as fh:
            meta = json.load(fh)
        # provider.py:254 + :354-359: OPENCV_FISHEYE scenes go through the un-distortion branch of the ray generator
        self.distortion = ([float(meta.get(k, 0.0)) for k in ("k1", "k2", "k3", "k4", "p1", "p2")]
                           if meta.get("camera_model") == "OPENCV_FISHEYE" else None)
        self.meta = meta
        frames = sorted(meta["frames"], key=lambda x: x["file_path"])                                  # provider.py:218
        poses = np.array([np.array(f["transform_matrix"]) for f in frames]).astype(np.float32)
        images_lis = [os.path.join(data_dir, f["file_path"]) for f in frames]
        masks_lis = [t.replace("images", keyword).replace(".jpg", ".png").replace(".JPG", ".png") for t in images_lis]
        poses, self.transform = auto_orient_and_center_poses(torch.tensor(poses), method="up", center_poses=True)
        poses = poses.numpy()
        poses[:, :3, 3] *= 1.0 / float(np.max(np.abs(poses[:, :3, 3])))                               # :233-236
        n = len(images_lis)
        i_train = np.linspace(0, n - 1, math.ceil(n * train_fraction), dtype=int)                      # :243-248
        self.image_paths = [images_lis[i] for i in i_train]
        self.mask_paths = [masks_lis[i] for i in i_train]
        self.camera_to_world = torch.from_numpy(poses[i_train][:, :3]).contiguous()
        self.split = split
        trajectory = split == 'test' and not dont_inter_test
        if trajectory:
            self.camera_to_world = trajectory_poses(self.camera_to_world, dis_scale)
            self.image_paths, self.mask_paths = [''] * len(self.camera_to_world), [''] * len(self.camera_to_world)
            load_images = False
        elif split == 'val' and not val_all_images:
            keep = key_view_indices(len(self.image_paths)).tolist()
            self.image_paths = [self.image_paths[i] for i in keep]
            self.mask_paths = [self.mask_paths[i] for i in keep]
            self.camera_to_world = self.camera_to_world[keep].contiguous()
        self.n_images = len(self.image_paths)
        self.fx, self.fy = focal_lengths(meta)
        self.cx, self.cy = float(meta["cx"]), float(meta["cy"])
        if load_images:
            imgs = [_load_image(p, resolution_level, "RGB") for p in self.image_paths]
            self.H, self.W = imgs[0].shape[0], imgs[0].shape[1]
            masks = []
            for p in self.mask_paths:
                if not os.path.isfile(p):
                    masks.append(np.zeros((self.H, self.W), np.float32))                               # :279-282
                    continue
                from PIL import Image
                m = Image.open(p).convert("L").resize((self.W, self.H), Image.BOX)
                m = np.asarray(m, dtype=np.float32) / 256.0
                masks.append((m > 0).astype(np.float32))                                               # mask[mask > 0] = True
            self.images = torch.from_numpy(np.stack(imgs)).to(device)                                  # [V,H,W,3]
            self.masks = torch.from_numpy(np.stack(masks)).to(device)                                  # [V,H,W]
        else:
            self.H, self.W = int(meta["h"] / resolution_level), int(meta["w"] / resolution_level)
            self.images = self.masks = None
        o, d = generate_rays(self.camera_to_world.to(device), self.fx, self.fy, self.cx, self.cy, self.H, self.W, float(resolution_level), "nerfstudio",
                             distortion=self.distortion)
        self.rays_o, self.rays_d = o.view(self.n_images, 1, -1, 3), d.view(self.n_images, 1, -1, 3)

    def __len__(self):
        return self.n_images

    def __getitem__(self, i):
        rgbs = self.images[i].reshape(1, -1, 3) if self.images is not None else None
        mask = self.masks[i].reshape(1, -1) if self.masks is not None else None
        return rgbs, mask, self.rays_o[i], self.rays_d[i], self.H, self.W, self.image_paths[i]
