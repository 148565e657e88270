"""Model-level drop-in for the reference's `GaussianSplattingRenderer` (gs/gaussian_splatting.py:68-1476) on the fused,
batched HIP path (VERDICT r4 missing #2 / next #3).

The reference's trainer reaches the rasterizer through ONE call, `renderer(batch, use_bg, rgb_only)`
(trainer.py:294 -> gs/gaussian_splatting.py:1423-1466), which loops over the cameras of the batch in Python
(render_one :1198-1421: frustum cull, five boolean-mask gathers, torch projection, AABB count with a `.item()` host sync,
binning + sort, render_with_T + three render_scalar passes) and stacks the per-camera dicts.  This class keeps that call --
the constructor arguments (cfg, initial_values), the parameter names (mean, qvec, svec_before_activation,
color_before_activation, alpha_before_activation: checkpoints load either way), the activations table
(utils/activations.py, conf/base.yaml:141-143), the buffers the densify / prune step reads (max_radii2d,
mean_2d_grad_accum, cnt, :464-479, :1240-1245), `forward(batch, use_bg=True, rgb_only=False)` returning the same dict
(`rgb` [B,H,W,3], `depth`, `opacity`, `z_var` [B,H,W,1]) and `post_backward()` -- and renders the whole batch with one enqueue
per stage (BatchRenderer.render_heads: rgb + depth + opacity + depth^2 in ONE compositing pass per direction, no mask gathers,
no host sync).  A user of the reference swaps

    from gs.gaussian_splatting import GaussianSplattingRenderer     ->     from gsgen_amd.model import GaussianSplattingRenderer

and, for the calls listed in INTEGRATION.md section 0 (the table of trainer.py lines), nothing else: setup_lr / set_optimizer /
optimizer / update / densify / prune / log / auxiliary_loss / bg(rays_d) exist since round 6.  The per-camera `_gs`
drop-in (gsgen_amd.install_as_gs) stays available for code that calls the 23 names directly, at the reference's serial shape
(bench.py reports both: `dropin_gs_surface` against `model_surface`).

What is NOT carried over (raises NotImplementedError when configured or called): pbr / specular shading (with normal_type "learned"),
overrides of anything but `color`, the pbr-only penalties (specular, normal) and `move`, the gradient-mask windows of update().
cfg.normal_as_rgb (conf/renderer/normal_as_rgb.yaml) renders: forward(batch) estimates the centres' normals (update_normal(), on
gsgen_amd.normals: pytorch3d's estimate_pointcloud_normals as one HIP launch, no autograd graph), renders them as the colour
override (normal + 1) / 2 and normalises every pixel (gs/gaussian_splatting.py:1424-1427, :1463-1464).  The learned
MLPBackground (background.type "mlp", tinycudann in the reference) runs on gsgen_amd.background.  Penalty losses and compatness densification take their neighbours from gsgen_amd.knn (the HIP kNN kernel).
The densify / prune policies themselves live in gsgen_amd.densify (this class delegates; AdaptiveControl is the multi-rank form on a
FusedAdam), the flat-buffer optimiser in gsgen_amd.optim.
"""
import numpy as np
import torch
import torch.nn as nn

from .batch import BatchRenderer

min_scale = 1e-3  # utils/activations.py:17

# utils/activations.py:36-57 (the tensor halves: the reference's wrappers also take python numbers)
activations = dict(
    abs=torch.abs, relu=torch.nn.functional.relu, sigmoid=torch.sigmoid, nothing=lambda x: x, exp=torch.exp,
    biased_relu=lambda x: torch.relu(x) + min_scale, biased_abs=lambda x: torch.abs(x) + min_scale,
    softplus=torch.nn.functional.softplus)
inv_activations = dict(
    abs=torch.abs, nothing=lambda x: x, sigmoid=torch.logit, relu=lambda x: x, exp=torch.log,
    biased_relu=lambda x: x - min_scale, biased_abs=lambda x: x - min_scale,
    softplus_inv=lambda x: x + torch.log(-torch.expm1(-x)))


def _get(cfg, key, default=None):
    """cfg nodes are OmegaConf nodes in the reference; dicts and attribute objects work too"""
    if cfg is None:
        return default
    if hasattr(cfg, "get"):
        try:
            return cfg.get(key, default)
        except Exception:
            pass
    return getattr(cfg, key, default)


def _to_plain(v):
    """OmegaConf nodes -> python containers (utils/misc.py:200-211), without importing omegaconf"""
    if v is None or isinstance(v, (int, float, str, list, dict)):
        return v
    try:
        from omegaconf import OmegaConf
        return OmegaConf.to_container(v, resolve=True)
    except Exception:
        return dict(v) if hasattr(v, "keys") else list(v)


def _lr_schedule(spec):
    """-> f(step) for one field of the trainer's `lr` config (gs/gaussian_splatting.py:267-292 over utils/schedulers.py:6-41 and
    utils/misc.py:218-260)"""
    if isinstance(spec, (int, float)):
        return lambda step, v=float(spec): v
    if not isinstance(spec, (list, tuple)) or len(spec) not in (4, 5):
        raise ValueError(f"Invalid lr schedule {spec}")
    if len(spec) == 4 and isinstance(spec[3], str):
        lr0, lr1, total, kind = float(spec[0]), float(spec[1]), float(spec[2]), spec[3]
        if kind == "nothing":
            return lambda step: lr0
        if kind == "exp":  # log-linear from lr_start to lr_end over max_steps
            return lambda step: float(np.exp(np.log(lr0) + (np.log(lr1) - np.log(lr0)) * min(max(step / total, 0.0), 1.0)))
        if kind == "cosine":
            return lambda step: lr1 + (lr0 - lr1) * (1.0 + float(np.cos(np.pi * step / total))) / 2.0
        raise ValueError(f"Invalid lr schedule {spec}")
    s0, v0, v1, s1 = (float(x) for x in spec[:4])  # piecewise: linear (or sqrt) from (s0, v0) to (s1, v1), constant outside
    root = len(spec) == 5 and spec[4] == "sqrt"

    def f(step):
        w = min(max((step - s0) / (s1 - s0), 0.0), 1.0)
        return v1 - (v1 - v0) * float(np.sqrt(w)) if root else v0 + (v1 - v0) * w
    return f


def schedule_value(spec, step, max_steps=None):
    """A scalar that may follow the training step -- how the reference's configs write penalty weights (utils/misc.py:218-260):
        number                                  constant
        [v0, v1, s1]                            the same as [0, v0, v1, s1]
        [s0, v0, v1, s1]                        linear from (s0, v0) to (s1, v1), constant outside
        [s0, v0, v1, s1, "linear" | "sqrt"]     that ramp, or v1 - (v1 - v0) * sqrt(t) with t the ramp's position in [0, 1]
    A float s1 is a fraction of max_steps; the reference then evaluates the ramp at step s1 * max_steps, and so does this."""
    if isinstance(spec, (int, float)):
        return spec
    spec = _to_plain(spec)
    if not isinstance(spec, list) or len(spec) not in (3, 4, 5):
        raise ValueError(f"gsgen_amd.model: a scheduled scalar is a number or a list of 3, 4 or 5 entries, not {spec!r}")
    if len(spec) == 3:
        spec = [0, *spec]
    s0, v0, v1, s1 = spec[:4]
    kind = spec[4] if len(spec) == 5 else "linear"
    if kind not in ("linear", "sqrt"):
        raise NotImplementedError(f"gsgen_amd.model: scheduled scalar of kind {kind!r} (linear and sqrt are supported)")
    at = step
    if kind == "linear" and isinstance(s1, float):
        if max_steps is None:
            raise ValueError(f"gsgen_amd.model: {spec!r} ends at a fraction of the run, which needs max_steps")
        at = s1 * max_steps
    t = max(min(1.0, (at - s0) / (s1 - s0)), 0.0)
    if kind == "sqrt":
        return v1 - (v1 - v0) * float(np.sqrt(t))
    return v0 + (v1 - v0) * t


class _Background(nn.Module):
    """gs/backgrounds.py: `fixed` (a constant colour held as a Parameter, :33-45), `random` (one torch.rand(3) per camera while
    training, black in eval, :48-70 -- drawn from torch's CPU generator exactly as the reference draws it, one draw per camera
    in batch order, so a seeded run sees the same colours), `learned_const` (:73-85).  -> [B, 1, 1, 3] for the batch.
    `mlp` (:88-114) is a colour per pixel: bg(rays_d), images(cams, B, H, W) and over(rgb, opacity, cams) on gsgen_amd.background; its
    768 parameters are `mlp.params`, the reference's state-dict key."""

    def __init__(self, cfg):
        super().__init__()
        self.type = _get(cfg, "type", "random")
        self.range = list(_get(cfg, "range", [0.0, 1.0]))
        self.random_aug = bool(_get(cfg, "random_aug", False)) and self.type != "fixed"  # (FixedBackground disables it, gs/backgrounds.py:44-45)
        self.random_aug_prob = float(_get(cfg, "random_aug_prob", 0.0))
        if self.type == "fixed":
            self.bg_color = nn.Parameter(torch.tensor(list(_get(cfg, "color")), dtype=torch.float32))
        elif self.type == "learned_const":
            self.bg_color = nn.Parameter(torch.tensor(list(_get(cfg, "initial_color", [0.5, 0.5, 0.5])), dtype=torch.float32))
        elif self.type == "mlp":
            # gs/backgrounds.py:88-114 on gsgen_amd.background (the reference's needs tinycudann): a colour per PIXEL, so the batched
            # forward goes through images() / over() below and not through forward(B)
            from .background import MLPBackground
            if self.random_aug:
                raise NotImplementedError("gsgen_amd.model: background.random_aug with type 'mlp' (conf/renderer/mlp_bg.yaml does not use it)")
            self.mlp = MLPBackground(None).mlp  # (the state dict key is `mlp.params`, as the reference's)
        elif self.type != "random":
            raise NotImplementedError(f"gsgen_amd.model: background type {self.type!r} (known: fixed, random, learned_const, mlp; pass the "
                                      "colours yourself through BatchRenderer.render_heads(bg_rgb=...))")
        # a captured step (gsgen_amd.graph.CapturedStep, model.device_cameras): the colours drawn on the host live in ONE device tensor
        # that the captured launches read; a forward enqueued into a capture draws nothing, refresh() draws for the next replay
        self.static = False
        self._static = None

    def forward(self, B, device=None):
        """B cameras -> [B, 1, 1, 3] (what the batched forward composites); or, called as the reference calls it -- bg(rays_d) with
        rays_d [H, W, 3], gs/gaussian_splatting.py:1321 -- -> [H, W, 3] for one camera"""
        if self.type == "mlp":
            if not isinstance(B, torch.Tensor):
                raise TypeError("gsgen_amd.model: an mlp background has a colour per pixel: call bg(rays_d), bg.images(cams, B, H, W) or "
                                "bg.over(rgb, opacity, cams)")
            from .background import mlp_background
            return mlp_background(self.mlp.params, B)
        if isinstance(B, torch.Tensor):
            rays = B
            return self.forward(1, rays.device).view(1, 1, 3).expand(rays.shape[0], rays.shape[1], 3).to(rays.dtype)
        if self.static and self.type == "random" and not self.random_aug:
            if torch.cuda.is_current_stream_capturing():
                if self._static is None or self._static.shape[0] < B:
                    raise RuntimeError("gsgen_amd.model: a random background inside a capture needs one eager forward of this batch size first")
                return self._static[:B]
            cols = self._colours(B, device)
            if self._static is None or self._static.shape[0] < B or self._static.device != cols.device:
                self._static = torch.empty(B, 1, 1, 3, device=cols.device, dtype=cols.dtype)
            self._static[:B].copy_(cols)
            return self._static[:B]
        if self.random_aug and self.training and self.type != "fixed":
            if self.static and torch.cuda.is_current_stream_capturing():
                raise NotImplementedError("gsgen_amd.model: random_aug backgrounds pick per camera on the host: not inside a captured step")
            # gs/backgrounds.py:24-36: with probability 1 - random_aug_prob a camera's background is one random colour
            import random
            cols = self._colours(B, device)
            pick = torch.tensor([random.random() >= self.random_aug_prob for _ in range(B)], device=cols.device)
            rnd = torch.stack([torch.rand(3) for _ in range(B)]).to(cols).view(B, 1, 1, 3)
            return torch.where(pick.view(B, 1, 1, 1), rnd, cols)
        return self._colours(B, device)

    def images(self, cams, B, H, W):
        """type 'mlp': -> [B, H, W, 3], the learned colour of every pixel of the B cameras whose blocks are the rows of cams"""
        from .background import mlp_background_images
        return mlp_background_images(self.mlp.params, cams[:B], H, W)

    def over(self, rgb, opacity, cams):
        """type 'mlp': -> rgb + (1 - opacity) * bg in one launch (gsgen_amd.background.mlp_background_over)"""
        from .background import mlp_background_over
        return mlp_background_over(self.mlp.params, rgb, opacity, cams)

    def _colours(self, B, device):
        if self.type == "random":
            if self.training:
                cols = torch.stack([torch.rand(3) for _ in range(B)])  # (CPU generator, one draw per camera: gs/backgrounds.py:58)
            else:
                cols = torch.zeros(B, 3)
            cols = cols.to(device) * (self.range[1] - self.range[0]) + self.range[0]
            return cols.view(B, 1, 1, 3)
        return self.bg_color.view(1, 1, 1, 3).expand(B, 1, 1, 3)


class _Stats:
    """the module's densify buffers in the shape BatchRenderer updates them (renderer.DensifyStats)"""

    def __init__(self, max_radii2d, grad_accum, cnt):
        self.max_radii2d, self.grad_accum, self.cnt = max_radii2d, grad_accum, cnt


class GaussianSplattingRenderer(nn.Module):
    """See the module docstring.  cfg: the `renderer` node of conf/base.yaml:129-171 (device, tile_size = 16, frustum_culling_radius,
    tile_culling_radius, T_thresh, svec_act / alpha_act / color_act, depth_detach, skip_frustum_culling, background, densify,
    prune).  initial_values: dict of mean [N,3], qvec [N,4], svec [N,3], color [N,3], alpha [N] (post-activation unless
    `raw` is set, gs/gaussian_splatting.py:171-205)."""

    def __init__(self, cfg, initial_values=None, strict=False, pipeline=False):
        super().__init__()
        self.cfg = cfg
        self.device = torch.device(_get(cfg, "device", "cuda"))
        if _get(cfg, "pbr", False):
            raise NotImplementedError("gsgen_amd.model: cfg.pbr is outside the rasterizer path this library replaces")
        self.normal_as_rgb = bool(_get(cfg, "normal_as_rgb", False))
        self.normal_type = _get(cfg, "normal_type", "estimated")  # gs/gaussian_splatting.py:75
        self._normal = None
        self._act_names = tuple(_get(cfg, k) for k in ("svec_act", "alpha_act", "color_act"))
        self.svec_act, self.alpha_act, self.color_act = (activations[_get(cfg, k)] for k in ("svec_act", "alpha_act", "color_act"))
        self.svec_inv_act, self.alpha_inv_act, self.color_inv_act = (
            inv_activations[_get(cfg, k)] for k in ("svec_act", "alpha_act", "color_act"))
        self.step = 0
        self.N = -1
        if initial_values is not None:
            self.initialize(initial_values)
        self.setup(cfg)
        self.masks, self.mean_2ds = [], []  # (the reference's per-camera bookkeeping for update_densify_info: stays empty here --
        # the fused backward accumulates the statistics itself)
        self._strict, self._pipeline = bool(strict), pipeline
        self.device_cameras = False  # True: camera blocks and pixel sizes from device memory (gsgen_amd.graph.CapturedStep)
        self._br = None
        self.to(self.device)

    # ---- fields (gs/gaussian_splatting.py:113-145, :171-205) ----------------------------------------------------------
    @property
    def svec(self):
        return self.svec_act(self.svec_before_activation)

    @property
    def alpha(self):
        return self.alpha_act(self.alpha_before_activation)

    @property
    def color(self):
        return self.color_act(self.color_before_activation)

    @svec.setter
    def svec(self, value):
        if value.shape == self.svec_before_activation.shape:
            self.svec_before_activation.data = self.svec_inv_act(value)
        else:
            self.svec_before_activation = nn.Parameter(self.svec_inv_act(value.data))

    @alpha.setter
    def alpha(self, value):
        if value.shape == self.alpha_before_activation.shape:
            self.alpha_before_activation.data = self.alpha_inv_act(value)
        else:
            self.alpha_before_activation = nn.Parameter(self.alpha_inv_act(value.data))

    @color.setter
    def color(self, value):
        if value.shape == self.color_before_activation.shape:
            self.color_before_activation.data = self.color_inv_act(value)
        else:
            self.color_before_activation = nn.Parameter(self.color_inv_act(value.data))

    def initialize(self, initial_values, raw=False):
        if "raw" in initial_values:
            raw = initial_values["raw"]
        self.mean = nn.Parameter(initial_values["mean"])
        self.qvec = nn.Parameter(initial_values["qvec"])
        inv = (lambda f, x: x) if raw else (lambda f, x: f(x))
        self.svec_before_activation = nn.Parameter(inv(self.svec_inv_act, initial_values["svec"]))
        self.color_before_activation = nn.Parameter(inv(self.color_inv_act, initial_values["color"]))
        self.alpha_before_activation = nn.Parameter(inv(self.alpha_inv_act, initial_values["alpha"]))
        self.N = self.mean.data.shape[0]

    def setup(self, cfg):
        self.tile_size = int(_get(cfg, "tile_size", 16))
        if self.tile_size != 16:
            raise NotImplementedError("gsgen_amd.model: the fused batched path is built for the reference's configured tile_size = 16 "
                                      "(conf/base.yaml:132); other sizes go through the per-camera `_gs` names")
        self.frustum_culling_radius = float(_get(cfg, "frustum_culling_radius", 6.0))
        self.tile_culling_radius = float(_get(cfg, "tile_culling_radius", 6.0))
        self.T_thresh = float(_get(cfg, "T_thresh", 1e-4))
        self.densify_cfg, self.prune_cfg = _get(cfg, "densify"), _get(cfg, "prune")
        self.densify_enabled = bool(_get(self.densify_cfg, "enabled", False))
        n = max(self.N, 0)
        self.register_buffer("max_radii2d", torch.zeros(n))
        if self.densify_enabled:
            self.register_buffer("mean_2d_grad_accum", torch.zeros(n))
            self.register_buffer("cnt", torch.zeros(n))
        self.depth_detach = bool(_get(cfg, "depth_detach", True))
        self.bg = _Background(_get(cfg, "background"))
        self.skip_frustum_culling = bool(_get(cfg, "skip_frustum_culling", False))
        self.fields = ["mean", "qvec", "svec", "color", "alpha"]
        self.raw_fields = ["mean", "qvec", "svec_before_activation", "color_before_activation", "alpha_before_activation"]

    def reset_densify_info(self):  # gs/gaussian_splatting.py:476-479
        self.mean_2d_grad_accum = torch.zeros_like(self.mean[..., 0])
        self.cnt = torch.zeros_like(self.mean_2d_grad_accum)
        self.max_radii2d = torch.zeros_like(self.mean_2d_grad_accum)

    # ---- rendering ----------------------------------------------------------------------------------------------------
    def _renderer(self, B, W, H):
        """the BatchRenderer of the current (N, W, H): rebuilt when the Gaussian set (densify / prune), the image size or the
        largest batch seen changes"""
        br = self._br
        same = (br is not None and (br.N, br.W, br.H) == (self.N, W, H) and br.device == self.mean.device
                and br.device_cameras == self.device_cameras)
        if not same or len(br.slots) < B:
            cap = max(B, len(br.slots)) if same else B
            br = self._br = BatchRenderer(self.N, W, H, self.mean.device, max_batch=cap, strict=self._strict,
                                          pipeline=self._pipeline, device_cameras=self.device_cameras)
        return br

    def prepare_replay(self, batch):
        """before the replay of a captured step (gsgen_amd.graph.CapturedStep calls it): what an eager forward does on the HOST for this
        batch and a capture cannot -- a random background's colours, drawn as the reference draws them (gs/backgrounds.py:58) and put
        where the captured launches read them"""
        self.bg.static = self.device_cameras
        if self.bg.type == "random" and self.bg.static:
            self.bg(len(batch["camera_info"]), self.mean.device)

    def batch_renderer(self, batch):
        """the BatchRenderer forward(batch) will use (gsgen_amd.graph.CapturedStep uploads a replay's cameras through it)"""
        infos = batch["camera_info"]
        return self._renderer(len(infos), int(infos[0].w), int(infos[0].h))

    def forward(self, batch, use_bg=True, rgb_only=False):
        """batch: {"c2w": [B, 3|4, 4] tensor (any device) or array, "camera_info": B CameraInfo-like objects (fx, fy, cx, cy, w, h,
        near_plane, far_plane: the reference's utils/camera.py:219-259 or gsgen_amd.renderer.CameraInfo)}.
        -> {"rgb": [B,H,W,3]} + {"depth", "opacity", "z_var": [B,H,W,1]} unless rgb_only (gs/gaussian_splatting.py:1423-1466).
        use_bg is accepted and ignored, as in the reference (:1324-1327: the background is always composited).
        With cfg.normal_as_rgb (:1424-1427, :1463-1464) the estimated normals are rendered in place of the colours, as
        (normal + 1) / 2, and every pixel is normalised afterwards: the view that shows the geometry a run has learnt.  The override
        is a constant; gradients reach mean / qvec / svec / alpha through the compositing."""
        if not self.normal_as_rgb:
            return self._render(batch, use_bg, rgb_only)
        out = self._render(batch, use_bg, rgb_only, color=(self.update_normal() + 1.0) * 0.5)
        out["rgb"] = (torch.nn.functional.normalize(out["rgb"], dim=-1, eps=1e-6) + 1.0) / 2.0
        return out

    # ---- normals (gs/gaussian_splatting.py:1186-1196) -------------------------------------------------------------------
    def _estimate_normal(self):
        if self.normal_type != "estimated":
            if self.normal_type == "learned":
                raise NotImplementedError("gsgen_amd.model: normal_type 'learned' belongs to pbr shading, which this class does not implement")
            raise ValueError(f"Unknown normal type: {self.normal_type}")
        from .normals import estimate_normal
        return estimate_normal(self.mean, **(_to_plain(_get(self.cfg, "normal")) or {}))

    def update_normal(self):
        """estimates the normals of the current centres with cfg.normal (neighborhood_size, disambiguate_directions) and keeps them
        for the render -> [N,3], no autograd graph (gsgen_amd.normals)"""
        self._normal = self._estimate_normal()
        return self._normal

    @property
    def normal(self):
        """the normals of the current centres, estimated at every read as the reference's property does"""
        return self._estimate_normal()

    def _render(self, batch, use_bg=True, rgb_only=False, color=None):
        """forward's render; color: [N,3] activated colours in place of the model's (render_one's overrides)"""
        c2ws = batch["c2w"]
        if isinstance(c2ws, torch.Tensor):
            c2ws = c2ws.detach().to("cpu", torch.float32).numpy()  # (poses come from the data loader on the host: no sync there)
        c2ws = np.ascontiguousarray(np.asarray(c2ws, np.float32))
        cis = list(batch["camera_info"])
        B = len(cis)
        W, H = int(cis[0].w), int(cis[0].h)
        if self.mean.shape[0] != self.N:
            self.N = self.mean.shape[0]
        br = self._renderer(B, W, H)
        stats = None
        if self.training:
            if self.max_radii2d.shape[0] != self.N:
                self.reset_densify_info()
            stats = _Stats(self.max_radii2d, self.mean_2d_grad_accum if self.densify_enabled else None,
                           self.cnt if self.densify_enabled else None)
        self.bg.static = self.device_cameras
        fr = 0.0 if self.skip_frustum_culling else self.frustum_culling_radius
        mlp_bg = self.bg.type == "mlp"
        if mlp_bg:
            # a learned colour per pixel (gsgen_amd.background), from the renderer's own camera blocks -- with device_cameras the
            # device ones, so a captured step's replay draws the background of the cameras then in place, with no upload of its own
            cams = br.camera_blocks(cis, c2ws, fr, self.tile_culling_radius)
            bg = self.bg.images(cams, B, H, W) if rgb_only else None
        else:
            bg = self.bg(B, self.mean.device)
        if color is not None and (not isinstance(color, torch.Tensor) or tuple(color.shape) != (self.N, 3)):
            raise ValueError(f"gsgen_amd.model: a colour override must be a [{self.N}, 3] tensor, got {getattr(color, 'shape', type(color))}")
        if rgb_only:
            rgb, _ = br.render(self.mean, self.qvec, self.svec, self.alpha, self.color if color is None else color, cis, c2ws, C=0,
                               bg_rgb=bg, thresh=self.T_thresh,
                               frustum_radius=fr, tile_radius=self.tile_culling_radius, detach_depth=self.depth_detach, stats=stats)
            return {"rgb": rgb}
        # (z_var = depth2 - depth^2, :1397, the background, gs/renderer.py:1182, and the three activations, :113-124, are formed inside
        # the launches / the batch's autograd node: round 6)
        # (an override is already activated: it goes through the launch's activation "nothing")
        acts = self._act_names if color is None else (self._act_names[0], self._act_names[1], "nothing")
        rgb, depth, opacity, z_var, _ = br.render_heads(self.mean, self.qvec, self.svec_before_activation, self.alpha_before_activation,
                                                        self.color_before_activation if color is None else color, cis, c2ws, bg_rgb=bg,
                                                        thresh=self.T_thresh, frustum_radius=fr, tile_radius=self.tile_culling_radius,
                                                        detach_depth=self.depth_detach, stats=stats, z_var=True,
                                                        activations=acts)
        if mlp_bg:
            # rgb + (1 - opacity) bg: opacity = sum alpha_i T_i telescopes to 1 - T, so this is gs/renderer.py:1182's rgb + T bg up to
            # rounding, and the Gaussians receive the background's d T / d alpha term through the opacity head's gradient
            rgb = self.bg.over(rgb, opacity, cams)
        return {"rgb": rgb, "depth": depth, "opacity": opacity, "z_var": z_var}

    def render_one(self, c2w, camera_info, use_bg=True, rgb_only=False, overrides=None, return_T=False):
        """gs/gaussian_splatting.py:1198-1421 for one camera (the viewer's and the evaluation loop's call): -> the same dict
        without the batch axis.  overrides: {"color": [N,3] activated colours} rendered in place of the model's (gradients flow to the
        tensor), gs/gaussian_splatting.py:1178-1183, :1224-1228."""
        color = None
        for k in (overrides or {}):
            if k != "color":
                raise NotImplementedError(f"gsgen_amd.model: overrides[{k!r}] (only the colour can be overridden)")
            color = overrides[k]
        c2w_np = c2w.detach().to("cpu", torch.float32).numpy() if isinstance(c2w, torch.Tensor) else np.asarray(c2w, np.float32)
        out = self._render({"c2w": c2w_np[None], "camera_info": [camera_info]}, use_bg, rgb_only, color=color)
        return {k: v[0] for k, v in out.items()}

    def post_backward(self):
        """gs/gaussian_splatting.py:1468-1473 -> update_densify_info :464-469.  The fused backward has already added every
        camera's |d L / d mean2d| and visit count to mean_2d_grad_accum / cnt (one masked pass behind the projection backward, on
        the render's stream): nothing is left to do here; the call stays so that the trainer's loop runs unchanged."""
        self.mean_2ds, self.masks = [], []

    def check_overflow(self):
        """no sync: raises PairListOverflow if a camera of an earlier batch did not fit its pair list (its images were NaN)"""
        return True if self._br is None else self._br.check_overflow()

    # ---- what trainer.py calls around the render (the class is only a drop-in if these exist) ------------------------
    # trainer.py:163-164, :230, :287, :469, :600-616, :800-801.  Optimiser and schedules follow gs/gaussian_splatting.py:267-292,
    # :383-419, :451-462 (one torch.optim group per field, named, lr re-evaluated every step); densify / prune delegate to
    # gsgen_amd.densify (the reference's policies :751-948, :1124-1177 restated there and tested against the reference's own code).
    def setup_lr(self, cfg):
        """cfg[field] for mean, qvec, svec, color, alpha, bg: a number, [lr_start, lr_end, max_steps, 'exp' | 'cosine' | 'nothing'], or
        the reference's piecewise form [start_step, start_value, end_value, end_step(, 'linear' | 'sqrt')] (utils/misc.py:218-260)"""
        for field in self.fields + ["bg"]:
            setattr(self, f"{field}_lr_scheduler", _lr_schedule(_to_plain(_get(cfg, field))))

    def get_param_groups(self):
        return {"mean": self.mean, "qvec": self.qvec, "svec": self.svec_before_activation, "color": self.color_before_activation,
                "alpha": self.alpha_before_activation, "bg": list(self.bg.parameters())}

    def set_optimizer(self, cfg, step=0):
        groups = []
        for name, params in self.get_param_groups().items():
            params = params if isinstance(params, list) else [params]
            if params:  # (a `random` background has no parameters: torch refuses an empty group)
                groups.append({"params": params, "lr": float(getattr(self, f"{name}_lr_scheduler")(step)), "name": name})
        self.opt_cfg = cfg
        args = _to_plain(_get(cfg, "opt_args")) or {}
        self.optimizer = getattr(torch.optim, _get(cfg, "type", "Adam"))(groups, lr=0.0, **args)

    def update_lr(self, step):
        for g in self.optimizer.param_groups:
            g["lr"] = float(getattr(self, f"{g['name']}_lr_scheduler")(step))

    def update(self, step):
        """trainer.py:287 (the reference also toggles its gradient mask here: `mask` configs are outside this class)"""
        self.step = step
        self.update_lr(step)

    @property
    def is_densifying(self):
        return self.densify_enabled

    def _raw(self):
        return {"mean": self.mean.data, "qvec": self.qvec.data, "svec": self.svec_before_activation.data,
                "color": self.color_before_activation.data, "alpha": self.alpha_before_activation.data}

    def _adopt(self, raw, moments=None, step=0):
        """new Gaussian set: Parameters, statistics, optimiser (fresh -- densify_legacy, :935 -- or with the surviving rows' Adam state)"""
        self.mean, self.qvec = nn.Parameter(raw["mean"]), nn.Parameter(raw["qvec"])
        self.svec_before_activation = nn.Parameter(raw["svec"])
        self.color_before_activation, self.alpha_before_activation = nn.Parameter(raw["color"]), nn.Parameter(raw["alpha"])
        self.N = self.mean.shape[0]
        if getattr(self, "optimizer", None) is not None:
            old_state = {g["name"]: self.optimizer.state.get(g["params"][0], None) for g in self.optimizer.param_groups}
            self.set_optimizer(self.opt_cfg, step)
            if moments is not None:
                for g in self.optimizer.param_groups:
                    k = g["name"]
                    if k in moments and old_state.get(k):
                        st = dict(old_state[k])
                        st["exp_avg"], st["exp_avg_sq"] = moments[k][0].contiguous(), moments[k][1].contiguous()
                        self.optimizer.state[g["params"][0]] = st

    def _moments(self):
        out = {}
        for g in getattr(self, "optimizer", None).param_groups if getattr(self, "optimizer", None) is not None else []:
            st = self.optimizer.state.get(g["params"][0], None)
            if g["name"] != "bg" and st and "exp_avg" in st:
                out[g["name"]] = (st["exp_avg"], st["exp_avg_sq"])
        return out

    @torch.no_grad()
    def densify(self, step, verbose=True):
        """gs/gaussian_splatting.py:751-948 through gsgen_amd.densify (`use_legacy`: split / clone from the accumulated screen-space
        gradient, the optimiser starts afresh; otherwise clone-then-split with the Adam state carried over)"""
        from . import densify as D
        c = self.densify_cfg
        if not (self.densify_enabled and _get(c, "warm_up", 0) <= step <= _get(c, "end", 0)
                and D.step_check(step, int(_get(c, "period", 1000)), True)):
            return 0
        kind = str(_get(c, "type", "official"))
        use_legacy = bool(_get(c, "use_legacy", True))
        dc = D.DensifyConfig(enabled=True, type="legacy" if use_legacy else "official",
                             warm_up=int(_get(c, "warm_up", 0)), end=int(_get(c, "end", 0)), period=int(_get(c, "period", 1000)),
                             mean2d_thresh=float(_get(c, "mean2d_thresh", 0.02)), split_thresh=float(_get(c, "split_thresh", 0.02)),
                             n_splits=int(_get(c, "n_splits", 2)), split_shrink=float(_get(c, "split_shrink", 0.8)))
        raw, n0 = self._raw(), self.N
        # :756-816: `use_legacy` runs the legacy split / clone and then the compatness step its type names; otherwise the type picks
        # one method ("scale" and "all" still take the official one here)
        compat = ("shrink_then_compatness" if "shrink_then_compatness" in kind else "compatness" if "compatness" in kind else None)
        if not use_legacy and kind not in ("compatness", "shrink_then_compatness"):
            compat = None
        info = {}
        if use_legacy or compat is None:
            if dc.type == "legacy":
                raw, info = D.densify_legacy(raw, self.svec.data, self.svec_inv_act, self.mean_2d_grad_accum, self.cnt, dc)
                moments = None
            else:
                raw, moments, info = D.densify_official(raw, self._moments(), {"svec": self.svec_act, "svec_inv": self.svec_inv_act},
                                                        self.mean_2d_grad_accum, self.cnt, dc)
            self._adopt(raw, moments, step)
        if compat == "shrink_then_compatness":
            info["num_compat"] = self.densify_by_shrink_then_compatness(float(_get(c, "surface_shrink", 1.5)), K=int(_get(c, "K", 3)))
        elif compat == "compatness":
            info["num_compat"] = self.densify_by_compatness(K=int(_get(c, "K", 3)))
        self.reset_densify_info()
        if verbose:
            print(f"[gsgen_amd] densify at step {step}: {n0} -> {self.N} Gaussians {info}")
        return self.N - n0

    @torch.no_grad()
    def prune(self, step, verbose=True):
        """gs/gaussian_splatting.py:1124-1177 (by screen-space radius, opacity, 3-D scale); the Adam state follows the survivors"""
        from . import densify as D
        c = self.prune_cfg
        if not (_get(c, "enabled", False) and _get(c, "warm_up", 0) <= step <= _get(c, "end", 0)
                and D.step_check(step, int(_get(c, "period", 500)))):
            return 0
        pc = D.PruneConfig(enabled=True, warm_up=int(_get(c, "warm_up", 0)), end=int(_get(c, "end", 0)), period=int(_get(c, "period", 500)),
                           radii2d_thresh=float(_get(c, "radii2d_thresh", 1000.0)), alpha_thresh=float(_get(c, "alpha_thresh", 1000.0)),
                           radii3d_thresh=float(_get(c, "radii3d_thresh", 0.0)))
        keep, counts = D.prune_masks(step, pc, self.max_radii2d, self.alpha.data, self.svec.data)
        n0 = self.N
        if bool(keep.all()):
            return 0
        stats = (self.max_radii2d[keep], self.mean_2d_grad_accum[keep] if self.densify_enabled else None,
                 self.cnt[keep] if self.densify_enabled else None)
        mom = {k: (a[keep], b[keep]) for k, (a, b) in self._moments().items()}
        self._adopt({k: v[keep] for k, v in self._raw().items()}, mom or None, step)
        self.max_radii2d = stats[0]
        if self.densify_enabled:
            self.mean_2d_grad_accum, self.cnt = stats[1], stats[2]
        if verbose:
            print(f"[gsgen_amd] prune at step {step}: {n0} -> {self.N} Gaussians {counts}")
        return n0 - self.N

    # ---- compatness densification (gs/gaussian_splatting.py:481-522, :634-743) -------------------------------------------------
    _raw_attr = {"mean": "mean", "qvec": "qvec", "svec": "svec_before_activation", "color": "color_before_activation",
                 "alpha": "alpha_before_activation"}

    @torch.no_grad()
    def densify_with_new_params(self, new_params):
        """:517-522 -> densify_on_optimizer :481-515: append the rows of new_params (raw fields) to every parameter; every non-`bg`
        optimiser group gets its parameter replaced and its Adam tensors extended with zeros (`step` is kept), the `bg` group is
        left alone.  The densify statistics are NOT reset here (densify() does that afterwards, :817)."""
        opt = getattr(self, "optimizer", None)
        groups = {g["name"]: g for g in opt.param_groups} if opt is not None else {}
        for name, attr in self._raw_attr.items():
            old = getattr(self, attr)
            ext = new_params[name].to(old.dtype)
            param = nn.Parameter(torch.cat((old.data, ext), dim=0).requires_grad_(True))
            g = groups.get(name)
            if g is not None:
                st = opt.state.pop(g["params"][0], None)
                if st is not None:
                    for k in list(st.keys()):
                        if torch.is_tensor(st[k]) and st[k].ndim != 0:
                            st[k] = torch.cat((st[k], torch.zeros_like(ext)), dim=0)
                    opt.state[param] = st
                g["params"][0] = param
            setattr(self, attr, param)
        self.N = self.mean.data.shape[0]

    @torch.no_grad()
    def densify_by_compatness(self, K=1):
        """:682-696: for each Gaussian and each of its K nearest other Gaussians (gsgen_amd.knn, a K + 1 search), a new Gaussian
        in the gap where the two surfaces do not touch; -> the number of new Gaussians"""
        from . import densify as D
        from .knn import K_nearest_neighbors
        _, idx = K_nearest_neighbors(self.mean.data, K=int(K) + 1)
        new = D.compatness_rows(self._raw(), self.svec.data, self.svec_inv_act, idx)
        self.densify_with_new_params(new)
        return new["mean"].shape[0]

    @torch.no_grad()
    def densify_by_shrink_then_compatness(self, shrink_factor, K=3):
        """:741-743: every scale divided by shrink_factor, then densify_by_compatness(K)"""
        self.svec = self.svec / shrink_factor
        return self.densify_by_compatness(K=K)

    # ---- penalty losses (gs/gaussian_splatting.py:950-1122) ------------------------------------------------------------------
    # Each _penalty_<key> returns the unweighted term (and extra scalars to log); auxiliary_loss weighs, logs and sums them.
    _PENALTY_KINDS = {"alpha": ("uniform_l1", "uniform_l2", "center_weighted"),
                      "mean": ("uniform_l1", "uniform_l2", "weighted_l1", "weighted_l2"), "compat": ("l1", "l2")}
    _PENALTY_UNSUPPORTED = {"move": "needs the previous step's means, which the reference never records",
                            "specular": "belongs to pbr shading, which this class does not implement",
                            "normal": "belongs to pbr shading, which this class does not implement"}

    def _penalty_node(self, key):
        return _get(_get(self.cfg, "penalty"), key)

    def _penalty_kind(self, key):
        kind = _get(self._penalty_node(key), "type")
        if kind not in self._PENALTY_KINDS[key]:
            raise ValueError(f"gsgen_amd.model: penalty.{key}.type is {kind!r}; expected one of {', '.join(self._PENALTY_KINDS[key])}")
        return kind

    def _penalty_alpha(self):
        """opacity: its mean, its mean square, or its mean weighted by the (constant) distance of each centre from the origin"""
        kind = self._penalty_kind("alpha")
        if kind == "center_weighted":
            return torch.mean(self.mean.detach().norm(dim=-1) * self.alpha), {}
        return torch.mean(self.alpha if kind == "uniform_l1" else self.alpha**2), {}

    def _penalty_mean(self):
        """distance of the centres from the origin: l1 / l2, optionally weighted by its own (constant) value"""
        kind = self._penalty_kind("mean")
        r = self.mean.norm(dim=-1)
        if kind == "uniform_l1":
            return torch.mean(r), {}
        if kind == "uniform_l2":
            return torch.mean(r**2), {}
        if kind == "weighted_l1":
            return torch.mean(r.detach() * self.mean.norm(dim=-1)), {}
        return torch.mean(r.detach() ** 2 * self.mean.norm(dim=-1) ** 2), {}

    def _penalty_scale(self):
        """summed volume (product of the three scales)"""
        return self.svec.prod(dim=-1).sum(), {}

    def _penalty_NN(self):
        """mean distance from each centre to its nearest other centre (the neighbour's position is a constant)"""
        from .knn import nearest_neighbor
        nn_pos, _ = nearest_neighbor(self.mean)
        return torch.mean((self.mean - nn_pos).norm(dim=-1)), {}

    def _penalty_compat(self):
        """mean over the Gaussians of the gap between their surface and their nearest neighbour's (zero where they touch), l1 or
        l2; the gradient flows through the gathered neighbour values"""
        from . import densify as D
        from .knn import nearest_neighbor
        kind = self._penalty_kind("compat")
        _, nb = nearest_neighbor(self.mean)
        dist, r_self, r_nb, _ = D.compat_gaps(self.mean, self.svec, D.rotmat_of_qvec(self.qvec), nb)
        gap_open = (r_self + r_nb) < dist
        gap = dist - r_self - r_nb
        term = torch.mean((gap if kind == "l1" else gap**2) * gap_open)
        return term, {"effective_rate": lambda: torch.sum(gap_open).item() / self.N}

    def auxiliary_loss(self, step, writer=None):
        """trainer.py:469 -> :1114-1122: the weighted sum of the penalties configured under cfg.penalty -- alpha, mean, scale, NN,
        compat, each weighted by schedule_value(<key>.value, step) and skipped at a weight <= 0 (scale: at 0).  NN and compat take
        their neighbours from gsgen_amd.knn without autograd.  With a writer the reference's scalars are logged
        (auxiliary/<key>_penalty, ..._weight, compat's effective_rate, total: each a host sync); without one nothing synchronises.
        `move` and the pbr-only `specular` / `normal` raise NotImplementedError when weighted."""
        loss = self.mean.new_zeros(())
        for key in list(_get(self.cfg, "penalty", None) or []):
            w = schedule_value(_get(self._penalty_node(key), "value", 0.0), step, None)
            if key in self._PENALTY_UNSUPPORTED:
                if w:
                    raise NotImplementedError(f"gsgen_amd.model: penalty {key!r} {self._PENALTY_UNSUPPORTED[key]}")
                continue
            term = getattr(self, f"_penalty_{key}", None)
            if term is None:
                raise ValueError(f"gsgen_amd.model: no penalty named {key!r}")
            if not (w != 0 if key == "scale" else w > 0):
                continue
            value, extra = term()
            if writer is not None:
                writer.add_scalar(f"auxiliary/{key}_penalty", value.item(), step)
                for name, get in extra.items():
                    writer.add_scalar(f"auxiliary/{name}", get(), step)
                writer.add_scalar(f"auxiliary/{key}_penalty_weight", w, step)
            loss = loss + w * value
        if writer is not None:
            writer.add_scalar("auxiliary/total", loss.item(), step)
        return loss

    @torch.no_grad()
    def log(self, writer, step):
        """trainer.py:603 / :841: scalars a TensorBoard-like writer takes (the reference logs bounds, gradient bounds, statistics,
        learning rates and the max_radii2d histogram, gs/gaussian_splatting.py:1477-1566)"""
        if writer is None:
            return
        writer.add_scalar("statistics/n_gaussians", self.N, step)
        for name, t in (("mean", self.mean), ("svec", self.svec), ("alpha", self.alpha)):
            writer.add_scalar(f"bounds/{name}_max", float(t.max()), step)
            writer.add_scalar(f"bounds/{name}_min", float(t.min()), step)
        for g in getattr(self, "optimizer", None).param_groups if getattr(self, "optimizer", None) is not None else []:
            writer.add_scalar(f"lr/{g['name']}", g["lr"], step)
        if hasattr(writer, "add_histogram"):
            writer.add_histogram("hists/max_radii2d", self.max_radii2d, step)

    @torch.no_grad()
    def get_density_val_grid(self, L=-1.0, reso=128, K=3):
        """utils/export.py:20-63 / gs/gaussian_splatting.py:1567: the density lattice of the mesh export from the model's activated
        fields (gsgen_amd.density: one fused search + sum launch) -> [reso,reso,reso] float32.  L < 0: mean.abs().max() * 1.1,
        one host sync as in the reference."""
        from .density import density_grid
        if L < 0.0:
            L = self.mean.abs().max().item() * 1.1
        return density_grid(self.mean, self.qvec, self.svec, self.alpha, L, reso, K, True)

    @torch.no_grad()
    def to_mesh(self, reso=128, K=3, thresh=0.5, L=-1.0, path=None):
        """utils/export.py:123-155 (`to_mesh`) from the model's activated fields, with vertex normals and colours ->
        (verts [V,3] world, tris [F,3] int32, normals [V,3], colors [V,3], L): gsgen_amd.mesh.colored_density_mesh on the field
        of get_density_val_grid.  L < 0: mean.abs().max() * 1.1 (one host sync).  path: also written there, `.obj`
        (gsgen_amd.io.write_obj) or `.ply` (write_ply_mesh) by its suffix."""
        import os
        from . import io as GIO
        from .mesh import colored_density_mesh
        if L < 0.0:
            L = self.mean.abs().max().item() * 1.1
        verts, tris, normals, colors = colored_density_mesh(self.mean, self.qvec, self.svec, self.alpha, self.color, L, reso, K,
                                                            thresh, True)
        if path is not None:
            suffix = os.path.splitext(str(path))[1].lower()
            if suffix not in (".obj", ".ply"):
                raise ValueError(f"gsgen_amd.model: to_mesh writes .obj or .ply, got {str(path)!r}")
            (GIO.write_obj if suffix == ".obj" else GIO.write_ply_mesh)(path, verts, tris, normals, colors)
        return verts, tris, normals, colors, L

    def get_params_for_save(self):  # gs/gaussian_splatting.py:294-311 (the five raw fields; gsgen_amd.io writes them)
        params = {k: getattr(self, k).detach() for k in self.raw_fields}
        if self.bg.type == "mlp":  # (:302: the learned background's state dict, key `mlp.params`)
            params["bg"] = self.bg.state_dict()
        return params
