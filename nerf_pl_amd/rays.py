"""Synthetic ray generation (restates ``datasets/ray_utils.py`` and the Blender /
LLFF camera conventions of ``datasets/blender.py`` / ``datasets/llff.py``).

These build the ``(N, 8) = [o, d, near, far]`` ray buffers the hot path
consumes.  They are plain tensor algebra on whatever device the inputs live on;
there is no dataset I/O (no data exists in this environment), so poses are
generated on a sphere like the reference's spheric render path
(``datasets/llff.py:128-149``).
"""
from __future__ import annotations

import math

import torch

LEGO_CAMERA_ANGLE_X = 0.6911112070083618   # nerf_synthetic/lego transforms_train.json


def blender_focal(img_w: int, camera_angle_x: float = LEGO_CAMERA_ANGLE_X) -> float:
    """datasets/blender.py:34-37: focal at 800 px, rescaled to ``img_w``."""
    return 0.5 * 800 / math.tan(0.5 * camera_angle_x) * img_w / 800


def get_ray_directions(H: int, W: int, focal: float, device=None) -> torch.Tensor:
    """ray_utils.py:5-24 -- camera-frame directions, no +0.5 pixel centering.
    ``i`` is the column (x) index and ``j`` the row (y) index, as kornia's
    ``create_meshgrid(H, W, normalized_coordinates=False)`` yields them."""
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=device),
                          torch.arange(W, dtype=torch.float32, device=device), indexing="ij")
    return torch.stack([(i - W / 2) / focal, -(j - H / 2) / focal, -torch.ones_like(i)], -1)


def get_rays(directions: torch.Tensor, c2w: torch.Tensor):
    """ray_utils.py:27-50 -- world-frame origins and unit directions."""
    rays_d = directions @ c2w[:, :3].T
    rays_d = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    rays_o = c2w[:, 3].expand(rays_d.shape)
    return rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)


def get_ndc_rays(H: int, W: int, focal: float, near: float, rays_o: torch.Tensor,
                 rays_d: torch.Tensor):
    """ray_utils.py:53-93 -- forward-facing (LLFF) NDC transform."""
    t = -(near + rays_o[..., 2]) / rays_d[..., 2]
    rays_o = rays_o + t[..., None] * rays_d
    ox_oz = rays_o[..., 0] / rays_o[..., 2]
    oy_oz = rays_o[..., 1] / rays_o[..., 2]
    o0 = -1. / (W / (2. * focal)) * ox_oz
    o1 = -1. / (H / (2. * focal)) * oy_oz
    o2 = 1. + 2. * near / rays_o[..., 2]
    d0 = -1. / (W / (2. * focal)) * (rays_d[..., 0] / rays_d[..., 2] - ox_oz)
    d1 = -1. / (H / (2. * focal)) * (rays_d[..., 1] / rays_d[..., 2] - oy_oz)
    d2 = 1 - o2
    return torch.stack([o0, o1, o2], -1), torch.stack([d0, d1, d2], -1)


def pose_spherical(theta_deg: float, phi_deg: float, radius: float) -> torch.Tensor:
    """(3,4) camera-to-world matrix looking at the origin from a sphere."""
    th, ph = math.radians(theta_deg), math.radians(phi_deg)
    trans = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1]],
                         dtype=torch.float64)
    rot_phi = torch.tensor([[1, 0, 0, 0],
                            [0, math.cos(ph), -math.sin(ph), 0],
                            [0, math.sin(ph), math.cos(ph), 0],
                            [0, 0, 0, 1]], dtype=torch.float64)
    rot_theta = torch.tensor([[math.cos(th), 0, -math.sin(th), 0],
                              [0, 1, 0, 0],
                              [math.sin(th), 0, math.cos(th), 0],
                              [0, 0, 0, 1]], dtype=torch.float64)
    flip = torch.tensor([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]],
                        dtype=torch.float64)
    c2w = flip @ rot_theta @ rot_phi @ trans
    return c2w[:3, :4].float()


def blender_rays(img_wh: int, n_poses: int, near: float = 1.0, far: float = 200.0,
                 radius: float = 4.0, phi_deg: float = -30.0, device=None) -> torch.Tensor:
    """Ray buffer (n_poses*H*W, 8) of a synthetic Blender-lego camera orbit.

    near/far default to this fork's Blender bounds (datasets/blender.py:40-41)."""
    H = W = img_wh
    focal = blender_focal(W)
    dirs = get_ray_directions(H, W, focal, device=device)
    out = []
    for k in range(n_poses):
        theta = -180.0 + 360.0 * k / n_poses
        c2w = pose_spherical(theta, phi_deg, radius).to(device)
        o, d = get_rays(dirs, c2w)
        nf = torch.tensor([near, far], dtype=torch.float32, device=device).expand(o.shape[0], 2)
        out.append(torch.cat([o, d, nf], 1))
    return torch.cat(out, 0)


def llff_ndc_rays(img_w: int = 504, img_h: int = 378, n_poses: int = 4,
                  focal: float = 407.0, device=None) -> torch.Tensor:
    """Forward-facing NDC rays (near/far 0/1) like datasets/llff.py:236-242."""
    dirs = get_ray_directions(img_h, img_w, focal, device=device)
    out = []
    for k in range(n_poses):
        ang = 2 * math.pi * k / max(n_poses, 1)
        c2w = torch.eye(4, dtype=torch.float32)[:3]
        c2w[:, 3] = torch.tensor([0.1 * math.cos(ang), 0.1 * math.sin(ang), 0.0])
        c2w = c2w.to(device)
        o, d = get_rays(dirs, c2w)                       # llff.py:234
        o_ndc, d_ndc = get_ndc_rays(img_h, img_w, focal, 1.0, o, d)   # llff.py:237-238
        nf = torch.tensor([0.0, 1.0], dtype=torch.float32, device=device).expand(o.shape[0], 2)
        out.append(torch.cat([o_ndc, d_ndc, nf], 1))
    return torch.cat(out, 0)


def _gen_rays(c2w, n_poses, H, W, focal, near, far, sel, n, ndc, ndc_near, rgb_pool):
    """the ``nr_gen_rays`` launch: (rays, rgb_out or None)"""
    from ._lib import call, ptr, stream_of
    dev = c2w.device
    rays = torch.empty(n, 8, device=dev)
    rgb_out = torch.empty(n, 3, device=dev) if rgb_pool is not None else None
    call("nr_gen_rays", ptr(c2w), n_poses, H, W, float(W / 2), float(H / 2), float(focal),
         float(near), float(far), int(ndc), float(ndc_near), -1. / (W / (2. * focal)),
         -1. / (H / (2. * focal)), 2. * ndc_near, ptr(sel), n, ptr(rgb_pool), ptr(rgb_out),
         ptr(rays), stream_of(dev))
    return rays, rgb_out


def pose_gradient(c2w: torch.Tensor, H: int, W: int, focal: float, g_rays: torch.Tensor,
                  sel: torch.Tensor = None, ndc: bool = False, ndc_near: float = 1.0,
                  with_focal: bool = False):
    """The transpose of ``generate_rays`` (``nr_gen_rays_posegrad``, DESIGN.md
    20): from ``g_rays`` (n, 8), the gradient of a loss in the rays that
    ``generate_rays(c2w, H, W, focal, ., ., sel, ndc, ndc_near)`` returned, the
    gradient in ``c2w`` (n_poses, 3, 4) and, ``with_focal``, one float64 focal
    partial per pose (n_poses), else None.  Columns 6..7 of ``g_rays`` are not
    read.  Deterministic: two calls give identical buffers."""
    from . import ops
    from ._lib import ptr, stream_of
    from ._lib_posegrad import call
    c2w = ops._dev(c2w.detach(), "c2w")
    if c2w.shape[-2:] != (3, 4):
        raise ValueError(f"c2w must be (n_poses, 3, 4), got {tuple(c2w.shape)}")
    dev = c2w.device
    n_poses = c2w.reshape(-1, 12).shape[0]
    if sel is not None:
        sel = sel.to(device=dev, dtype=torch.int64).contiguous()
    n = sel.shape[0] if sel is not None else n_poses * H * W
    g_rays = ops._dev(g_rays, "g_rays", 8)
    if g_rays.shape != (n, 8):
        raise ValueError(f"g_rays must be ({n}, 8), got {tuple(g_rays.shape)}")
    if g_rays.data_ptr() % 16:
        g_rays = g_rays.clone()
    if n == 0:      # an empty tensor has no address to pass; the gradient of no ray is zero
        return (torch.zeros(n_poses, 3, 4, device=dev),
                torch.zeros(n_poses, dtype=torch.float64, device=dev) if with_focal else None)
    g_c2w = torch.empty(n_poses, 3, 4, device=dev)
    g_focal = torch.empty(n_poses, dtype=torch.float64, device=dev) if with_focal else None
    focal = float(focal)
    call("nr_gen_rays_posegrad", ptr(c2w), n_poses, H, W, float(W / 2), float(H / 2), focal,
         int(ndc), float(ndc_near), -1. / (W / (2. * focal)), -1. / (H / (2. * focal)),
         2. * ndc_near, ptr(sel), n, ptr(g_rays), ptr(g_c2w), ptr(g_focal), stream_of(dev))
    return g_c2w, g_focal


class _GenRays(torch.autograd.Function):
    """``nr_gen_rays`` as a function of the poses and the focal length: the
    forward is the launch of the plain path (same rays, bit for bit), the
    backward is ``nr_gen_rays_posegrad``."""

    @staticmethod
    def forward(ctx, c2w, focal_t, focal, H, W, near, far, sel, ndc, ndc_near, rgb_pool):
        n_poses = c2w.reshape(-1, 12).shape[0]
        n = sel.shape[0] if sel is not None else n_poses * H * W
        rays, rgb_out = _gen_rays(c2w, n_poses, H, W, focal, near, far, sel, n, ndc, ndc_near,
                                  rgb_pool)
        ctx.save_for_backward(c2w, sel)
        ctx.geom = (H, W, focal, ndc, ndc_near)
        ctx.focal_meta = None if focal_t is None else (focal_t.device, focal_t.shape)
        if rgb_out is not None:
            ctx.mark_non_differentiable(rgb_out)
        return rays, rgb_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rays, _g_rgb):
        c2w, sel = ctx.saved_tensors
        H, W, focal, ndc, ndc_near = ctx.geom
        want_c2w, want_focal = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_c2w, g_focal = pose_gradient(c2w, H, W, focal, g_rays, sel, ndc, ndc_near,
                                       with_focal=want_focal)
        if want_focal:      # the float64 sum of the per-pose partials
            device, shape = ctx.focal_meta
            g_focal = g_focal.sum().to(torch.float32).to(device).reshape(shape)
        return (g_c2w.reshape(c2w.shape) if want_c2w else None, g_focal) + (None,) * 9


def generate_rays(c2w: torch.Tensor, H: int, W: int, focal: float, near: float, far: float,
                  sel: torch.Tensor = None, ndc: bool = False, ndc_near: float = 1.0,
                  rgb_pool: torch.Tensor = None):
    """Rays (n, 8) for global pixel indices ``sel`` (pose*H*W + row*W + col) of
    the poses ``c2w`` (n_poses, 3, 4), generated on the device by
    ``nr_gen_rays`` -- the batch the reference assembles from its precomputed
    ray buffer (datasets/blender.py:54-86, llff.py:213-249).  ``sel=None``
    means every pixel of every pose.  With ``rgb_pool`` (n_poses*H*W, 3) the
    target colours of the same pixels are returned too.  With ``ndc`` the
    forward-facing transform (get_ndc_rays, near plane ``ndc_near``) is applied
    and near/far become 0/1 (llff.py:236-242).

    The rays differentiate in the poses, as the reference's ``get_rays`` /
    ``get_ndc_rays`` do: when ``c2w`` requires grad (an ``nn.Parameter``, or any
    ``c2w = f(params)`` composed in torch) the same launch runs inside an
    ``autograd.Function`` whose backward is ``nr_gen_rays_posegrad`` (DESIGN.md
    20).  ``focal`` may also be a one-element float32 tensor; if it requires
    grad it receives the float64 sum of the per-pose partials.  Its value is
    read once on the host for the kernel's scalar arguments, so a
    device-resident focal costs a synchronisation per call: keep it a CPU
    scalar parameter.  Colours (``rgb_out``) carry no gradient.  When neither
    requires grad nothing new runs and ``rays.grad_fn`` is None."""
    from . import ops
    focal_t = None
    if isinstance(focal, torch.Tensor):
        if focal.numel() != 1 or focal.dtype != torch.float32:
            raise TypeError("focal: a float or a one-element float32 tensor, got "
                            f"{tuple(focal.shape)} {focal.dtype}")
        focal_t, focal = focal, focal.item()
    c2w = ops._dev(c2w.to(torch.float32), "c2w")
    if c2w.shape[-2:] != (3, 4):
        raise ValueError(f"c2w must be (n_poses, 3, 4), got {tuple(c2w.shape)}")
    dev = c2w.device
    n_poses = c2w.reshape(-1, 12).shape[0]
    if sel is not None:
        sel = sel.to(device=dev, dtype=torch.int64).contiguous()
        n = sel.shape[0]
    else:
        n = n_poses * H * W
    if rgb_pool is not None:
        rgb_pool = ops._dev(rgb_pool, "rgb_pool", 3)
    if ndc:
        near, far = 0.0, 1.0
    if torch.is_grad_enabled() and (c2w.requires_grad
                                    or (focal_t is not None and focal_t.requires_grad)):
        rays, rgb_out = _GenRays.apply(c2w, focal_t, focal, H, W, near, far, sel, ndc, ndc_near,
                                       rgb_pool)
    else:
        rays, rgb_out = _gen_rays(c2w, n_poses, H, W, focal, near, far, sel, n, ndc, ndc_near,
                                  rgb_pool)
    return (rays, rgb_out) if rgb_pool is not None else rays


class RaySampler:
    """Shuffled training batches generated on the device -- replaces the
    reference's ray buffer + ``DataLoader(shuffle=True, batch_size=B)``
    (train.py:89-94): each epoch is a random permutation of all pixels of all
    poses, each batch is produced by one ``nr_gen_rays`` launch that also
    gathers the target colours.

    Data-parallel runs partition every epoch like the ``DistributedSampler``
    that Lightning's DDP backend installs (train.py:175), and with
    its very permutation: ``torch.randperm`` of the epoch on a CPU generator
    seeded ``seed + epoch`` (identical on every rank), padded with its head to a
    multiple of ``world``, rank r taking ``perm[r::world]`` -- the ranks'
    batches are disjoint and together cover the epoch.  An epoch ends when the
    rank's shard cannot fill another batch (the remainder is dropped).  The
    permutation is drawn on the host by a worker thread one epoch ahead and
    only the rank's shard is copied to the device: a device-side randperm of a
    64M-pixel pool (cfg4) costs every rank a 64M-key radix sort per epoch, and
    with several ranks sharing one GPU (the one-GPU rehearsal of the 8-GPU
    run) four concurrent sorts did not finish in 100 s."""

    def __init__(self, c2w, H, W, focal, near, far, rgb_pool=None, ndc=False, seed=0, rank=0,
                 world=1):
        if not 0 <= rank < world:
            raise ValueError(f"RaySampler: rank {rank} outside world {world}")
        self.c2w = c2w
        self.H, self.W, self.focal, self.near, self.far = H, W, focal, near, far
        self.rgb_pool, self.ndc = rgb_pool, ndc
        self.total = c2w.reshape(-1, 12).shape[0] * H * W
        self.seed, self.rank, self.world = seed, rank, world
        self.device = c2w.device
        self.epoch, self.shard, self.pos = -1, None, 0
        self._pool = None
        self._ahead = None      # (epoch, future of its host shard)

    def _host_shard(self, epoch):
        gen = torch.Generator().manual_seed(self.seed + epoch)
        perm = torch.randperm(self.total, generator=gen)
        pad = (-self.total) % self.world          # DistributedSampler(drop_last=False)
        if pad:
            perm = torch.cat([perm, perm[:pad]])
        shard = perm[self.rank::self.world].contiguous()
        return shard.pin_memory() if self.device.type == "cuda" else shard

    def _new_epoch(self):
        import concurrent.futures
        self.epoch += 1
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
        if self._ahead is not None and self._ahead[0] == self.epoch:
            host = self._ahead[1].result()
        else:
            host = self._host_shard(self.epoch)
        self._ahead = (self.epoch + 1, self._pool.submit(self._host_shard, self.epoch + 1))
        self.shard = host.to(self.device, non_blocking=True)
        self.pos = 0

    def next_indices(self, batch: int):
        """Global pixel indices of the next batch (pose*H*W + row*W + col)."""
        if self.shard is None or self.pos + batch > self.shard.shape[0]:
            self._new_epoch()
            if batch > self.shard.shape[0]:
                raise ValueError(f"RaySampler: batch {batch} exceeds the rank's "
                                 f"{self.shard.shape[0]} rays per epoch")
        sel = self.shard[self.pos:self.pos + batch]
        self.pos += batch
        return sel

    def next(self, batch: int):
        sel = self.next_indices(batch)
        return generate_rays(self.c2w, self.H, self.W, self.focal, self.near, self.far, sel,
                             self.ndc, rgb_pool=self.rgb_pool)
