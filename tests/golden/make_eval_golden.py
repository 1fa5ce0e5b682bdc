"""Record tests/golden/inter_pose.npz from the REFERENCE's own inter_pose_num (nerf/provider.py:31-60), which goes through scipy's Slerp.

Run once where the reference tree and scipy exist (neither is needed by the tests):

    python tests/golden/make_eval_golden.py

Nothing of the reference travels: the file holds the input pose pairs, the scales and the poses the reference returned.  Modules the
reference's provider imports but this recording never calls (cv2) are replaced by empty stubs.

Cases (pose pairs are camera-to-world, rotation from a rotation vector, |translation| <= 1 as the loader's scaling leaves them):
    general    two unrelated rotations
    same_rot   identical rotations, different translations (the slerp's zero-angle branch)
    turn179    the second rotation is the first turned by 179 degrees about a skew axis (the long way round is 181: shortest-arc choice)
    scaled     general rotations with scale (0.5, 1.25, 2.0): unequal components
Each with num = 7 ratios, 0 and 1 included.
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("CUSTOMNERF_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))


def import_reference_provider():
    for name in ("cv2",):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    if "torchtyping" not in sys.modules:
        class _TT:
            def __class_getitem__(cls, item):
                return cls
        sys.modules["torchtyping"] = types.ModuleType("torchtyping")
        sys.modules["torchtyping"].TensorType = _TT
    sys.path.insert(0, REF)
    from nerf import provider
    return provider


def rot(rotvec):
    """Rodrigues, float64"""
    v = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def pose(R, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m.astype(np.float32)


def cases():
    r0, r1 = rot([0.3, -0.8, 0.5]), rot([-1.1, 0.4, 1.7])
    axis = np.array([0.6, -0.2, 0.77]) / np.linalg.norm([0.6, -0.2, 0.77])
    return {
        "general": (pose(r0, [0.9, -0.3, 0.2]), pose(r1, [-0.4, 0.8, 0.55]), 1.0),
        "same_rot": (pose(r0, [0.1, 0.7, -0.6]), pose(r0, [-0.8, 0.2, 0.3]), 1.0),
        "turn179": (pose(r1, [0.5, 0.5, -0.5]), pose(r1 @ rot(axis * np.deg2rad(179.0)), [-0.2, -0.9, 0.4]), 1.0),
        "scaled": (pose(r1, [0.9, -0.3, 0.2]), pose(r0, [-0.4, 0.8, 0.55]), np.array([0.5, 1.25, 2.0])),
    }


def main():
    provider = import_reference_provider()
    out = {}
    for name, (p0, p1, scale) in cases().items():
        got = provider.inter_pose_num(torch.from_numpy(p0), torch.from_numpy(p1), 7, scale=scale)
        out[name + "__pose_0"], out[name + "__pose_1"] = p0, p1
        out[name + "__scale"] = np.asarray(scale, np.float64)
        out[name + "__poses"] = got.numpy().astype(np.float32)
    path = os.path.join(HERE, "inter_pose.npz")
    np.savez(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items() if k.endswith("__poses")})


if __name__ == "__main__":
    main()
