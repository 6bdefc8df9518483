"""Rigs and a renderer for the rectification tests -- test infrastructure only.

The rig is pipeline.py's (the reference's calibration) at 1/3 scale, 320 x 200, with the rotation
of its stereo extrinsic multiplied by a factor: x4 (1.9 degrees) is an ordinary hand-assembled
rig on which the unrectified path fails.  The scene is a textured plane at z = 2.7 m in the
left camera's frame (optionally with a smooth relief), rendered through each raw (distorted, unrectified) camera by inverting
the distortion per pixel; the texture is seeded."""
import numpy as np

W, H, D = 320, 200, 64
Z0 = 2.7


def rodrigues(r):
    th = np.linalg.norm(r)
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * kx


def rotation_vector(R):
    c = (np.trace(R) - 1) / 2
    th = np.arccos(np.clip(c, -1, 1))
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return v * (0.5 if th < 1e-12 else th / (2 * np.sin(th)))


def rig(rotation_factor=4.0, scale=1 / 3.0):
    """(K_left, dist_left, K_right, dist_right, R, T) with x_right = R x_left + T."""
    from forest_slam_amd import pipeline as pl
    s = np.array([[scale], [scale], [1.0]])
    M = np.linalg.inv(pl.T_RGB0_RGB1.reshape(4, 4))
    R = rodrigues(rotation_vector(M[:3, :3]) * rotation_factor)
    return pl.K0 * s, pl.DIST_L.astype(np.float64), pl.K1 * s, pl.DIST_R.astype(np.float64), R, M[:3, 3].copy()


def vertical_rig():
    Kl, dl, Kr, dr, _, _ = rig()
    return Kl, dl, Kr, dr, rodrigues(np.array([0.02, -0.015, 0.03])), np.array([0.004, -0.21, 0.006])


def translation_rig():
    Kl, dl, Kr, dr, _, _ = rig()
    return Kl, dl, Kr, dr, np.eye(3), np.array([-0.25, 0.0, 0.0])


def rotz(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def lens_case(name, rect=None):
    """(K, dist, R, newK) of the tile-path cases at W x H: "aligned" = the x4 rig's left camera
    under its rectification `rect` (every tile staged), "rolled" = a 30 degree roll about z
    (tiles on both paths with 3 channels)."""
    Kl, dl, Kr, dr, R, T = rig()
    if name == "aligned":
        return Kl, dl, rect.R1, rect.P1[:, :3]
    if name == "rolled":
        return Kl, dl, rotz(30.0), Kl
    raise KeyError(name)


def scatter_map(seed=5):
    """A random-permutation map for remap (every tile gathers directly): (map1, map2)."""
    rng = np.random.default_rng(seed)
    p = rng.permutation(W * H)
    map1 = np.stack([(p % W).reshape(H, W), (p // W).reshape(H, W)], axis=-1).astype(np.int16)
    return map1, rng.integers(0, 1024, (H, W)).astype(np.uint16)


def undistort_points(u, v, K, d, iterations=30):
    xd, yd = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    x, y = xd.copy(), yd.copy()
    k1, k2, p1, p2, k3 = d[:5]
    for _ in range(iterations):
        r2 = x * x + y * y
        ik = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        x, y = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) * ik, (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) * ik
    return x, y


class Scene:
    def __init__(self, seed=0, cells_per_m=100.0, relief=0.0):
        """cells_per_m: texture cells per metre (100: finer than a pixel, the SGBM scene; ~20:
        corners a few pixels wide that ORB can follow from frame to frame).  relief: amplitude in
        metres of a smooth height field on the plane (PnP needs points that are not coplanar)."""
        from numpy.lib.stride_tricks import sliding_window_view
        self.cpm, self.relief = float(cells_per_m), float(relief)
        tex = np.random.default_rng(seed).integers(0, 256, (600, 900)).astype(np.float64)
        self.tex = sliding_window_view(np.pad(tex, 1, mode="wrap"), (3, 3)).mean((2, 3))

    def texture(self, X, Y):
        a, b = (X + 4.5) * self.cpm, (Y + 3) * self.cpm
        a0, b0 = np.floor(a).astype(int), np.floor(b).astype(int)
        fa, fb = a - a0, b - b0
        g = lambda yy, xx: self.tex[np.clip(yy, 0, 599), np.clip(xx, 0, 899)]
        return g(b0, a0) * (1 - fa) * (1 - fb) + g(b0, a0 + 1) * fa * (1 - fb) + g(b0 + 1, a0) * (1 - fa) * fb + \
            g(b0 + 1, a0 + 1) * fa * fb

    def render(self, K, d, Rc, Tc, width=W, height=H):
        """u8 [height, width]: the plane z = Z0 of the scene frame seen by the raw camera
        x_cam = Rc x_scene + Tc."""
        v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
        x, y = undistort_points(u, v, K, d)
        dirs = np.einsum("ij,jhw->ihw", Rc.T, np.stack([x, y, np.ones_like(x)]))
        o = -Rc.T @ Tc
        P = o[:, None, None] + ((Z0 - o[2]) / dirs[2]) * dirs
        if self.relief:  # ray / height-field intersection by fixed-point iteration (gentle slopes)
            for _ in range(30):
                z = Z0 + self.relief * np.sin(2.0 * P[0] + 0.3) * np.cos(2.0 * P[1] - 0.2)
                P = o[:, None, None] + ((z - o[2]) / dirs[2]) * dirs
        return np.clip(np.rint(self.texture(P[0], P[1])), 0, 255).astype(np.uint8)

    def stereo_pair(self, Kl, dl, Kr, dr, R, T, Rc=None, Tc=None):
        """The raw left and right images of the rig whose left camera is x_left = Rc x_scene + Tc."""
        Rc = np.eye(3) if Rc is None else Rc
        Tc = np.zeros(3) if Tc is None else Tc
        return self.render(Kl, dl, Rc, Tc), self.render(Kr, dr, R @ Rc, R @ Tc + T)


def region():
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return (u >= D + 8) & (u < W - 8) & (v >= 8) & (v < H - 8), u, v


def share_within_1px(disp16, truth):
    """Share of the region's pixels with a true disparity in (0, D - 1) whose int16 disparity
    (x16) is valid and within 1 px of it."""
    reg, _, _ = region()
    ok = reg & np.isfinite(truth) & (truth > 0) & (truth < D - 1)
    good = ok & (disp16 >= 0) & (np.abs(disp16.astype(np.float64) / 16 - truth) <= 1.0)
    return good.sum() / ok.sum()


def plane_depth_unrectified(Kl):
    """Per left pixel (undistorted with its own K), the plane point in the left frame."""
    _, u, v = region()
    dirs = np.stack([(u - Kl[0, 2]) / Kl[0, 0], (v - Kl[1, 2]) / Kl[1, 1], np.ones_like(u)])
    return (Z0 / dirs[2]) * dirs


def truth_unrectified(Kl, Kr, R, T):
    """Geometric disparity u_left - u_right of the undistort-only pair, and the vertical offset."""
    _, u, v = region()
    P = plane_depth_unrectified(Kl)
    Pr = np.einsum("ij,jhw->ihw", R, P) + T[:, None, None]
    ur, vr = Kr[0, 0] * Pr[0] / Pr[2] + Kr[0, 2], Kr[1, 1] * Pr[1] / Pr[2] + Kr[1, 2]
    return u - ur, v - vr


def truth_rectified(R1, P1, baseline):
    """fc * B / Z_rect per rectified-left pixel."""
    _, u, v = region()
    f = P1[0, 0]
    dirs = np.einsum("ij,jhw->ihw", R1.T, np.stack([(u - P1[0, 2]) / f, (v - P1[1, 2]) / f, np.ones_like(u)]))
    Pl = (Z0 / dirs[2]) * dirs
    return f * baseline / np.einsum("ij,jhw->ihw", R1, Pl)[2]
