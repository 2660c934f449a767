"""Loss modules with the reference's names/signatures (muvo/losses.py:53-287) on the fused HIP loss kernels.
`WorldModelTrainer.compute_loss` uses the fused multi-part entry points directly; these classes exist so code
written against the reference's loss objects keeps working."""
import torch
import torch.nn as nn

from muvo_amd import ops

VOXEL_SEG_WEIGHTS = (1.0, 1.0, 1.0, 1.5, 2.0, 3.0, 1.0, 1.0, 1.0)      # constants.py:39
SEMANTIC_SEG_WEIGHTS = (1.0, 1.0, 1.0, 2.0, 3.0, 1.0, 1.0, 1.0)        # constants.py:33


class RegressionLoss(nn.Module):
    """muvo/losses.py:53-71: |d| (norm 1) or d^2 (norm 2) summed over the channel dimension, mean over the rest."""

    def __init__(self, norm, channel_dim=-1):
        super().__init__()
        if norm not in (1, 2):
            raise ValueError(f'Expected norm 1 or 2, but got norm={norm}')
        if channel_dim != -1:
            raise NotImplementedError('the reference only ever uses the last dimension (trainer.py:57)')
        self.norm = norm

    def forward(self, prediction, target):
        if self.norm == 1:
            return ops.l1_rows_loss(prediction, target, 1.0)[0]
        # norm 2 on the masked spatial-loss kernel: rows = "frames" of one pixel, every row counted (all-ones mask)
        rows = prediction.numel() // prediction.shape[-1]
        p = prediction.reshape(1, rows, prediction.shape[-1], 1, 1)
        t = target.reshape(1, rows, prediction.shape[-1], 1, 1).float()
        ones = torch.ones(1, rows, 1, 1, 1, device=p.device, dtype=torch.uint8)
        return ops.spatial_losses(p, t, [(0, prediction.shape[-1], 2, 1.0)], mask=ones)[0]


class SpatialRegressionLoss(nn.Module):
    def __init__(self, norm, ignore_index=255):
        super().__init__()
        if norm not in (1, 2):
            raise ValueError(f'Expected norm 1 or 2, but got norm={norm}')
        self.norm, self.ignore_index = norm, ignore_index

    def forward(self, prediction, target, instance_mask=None):
        assert prediction.dim() == 5, 'Must be a 5D tensor'
        c = prediction.shape[2]
        return ops.spatial_losses(prediction, target, [(0, c, self.norm, 1.0)], float(self.ignore_index), mask=instance_mask)[0]


class KLLoss(nn.Module):
    def __init__(self, alpha):
        super().__init__()
        self.alpha = alpha

    def forward(self, prior, posterior):
        return ops.kl_loss(prior['mu'], prior['sigma'], posterior['mu'], posterior['sigma'], 1.0, self.alpha)[0]


class _VoxelTriple(nn.Module):
    index = 0

    def __init__(self, *a, **k):
        super().__init__()

    def forward(self, prediction, target):
        return ops.voxel_losses(prediction, target, 1.0)[self.index]


class VoxelLoss(_VoxelTriple):
    """muvo/losses.py:144-186.  Plain / class-weighted mean: the fused voxel-loss kernel.  Top-k: the per-voxel (weighted) cross
    entropy map from the segmentation kernels, `topk` over every frame's voxels (a selection), mean."""
    index = 0

    def __init__(self, use_top_k=False, top_k_ratio=1.0, use_weights=False, poly_one=False, poly_one_coefficient=0.0):
        super().__init__()
        if poly_one:
            raise NotImplementedError('poly-1 is never enabled by the reference trainer (trainer.py:163-170)')
        self.use_top_k, self.top_k_ratio = use_top_k, top_k_ratio
        self.weights = VOXEL_SEG_WEIGHTS if use_weights else None

    def forward(self, prediction, target):
        cw = torch.tensor(self.weights, dtype=torch.float32, device=prediction.device) if self.weights is not None else None
        if cw is not None and prediction.shape[2] != len(self.weights):
            raise ValueError(f'VOXEL_SEG.USE_WEIGHTS needs the {len(self.weights)}-class head (constants.py:39), got {prediction.shape[2]} classes')
        if not self.use_top_k:
            return ops.voxel_losses(prediction, target, 1.0, cw)[0]
        b, s, c = prediction.shape[:3]
        loss = ops.seg_ce_pixel_loss(prediction.reshape(b * s, c, -1), target.reshape(b * s, -1), cw).view(b, s, -1)
        k = int(self.top_k_ratio * loss.shape[2])
        return torch.mean(loss.topk(k, dim=-1)[0])


class SemScalLoss(_VoxelTriple):
    index = 1


class GeoScalLoss(_VoxelTriple):
    index = 2


class LovaszSoftmaxLoss(nn.Module):
    """Lovasz-softmax loss of voxel logits (b, s, c, x, y, z) against uint8 labels (b, s, 1, x, y, z): the convex surrogate of
    the Jaccard index, every frame a segment of its own, classes 'present' (not in the reference).
    Labels >= c - `ignore_index` among them - take no part."""

    def __init__(self, ignore_index=255):
        super().__init__()
        self.ignore_index = ignore_index

    def forward(self, prediction, target):
        if prediction.dim() != 6 or target.dim() != 6:
            raise ValueError(f'Expected 6-D logits and labels, got {tuple(prediction.shape)} and {tuple(target.shape)}')
        if self.ignore_index < prediction.shape[2]:
            raise ValueError(f'ignore_index {self.ignore_index} is one of the {prediction.shape[2]} classes: the kernels ignore labels >= C')
        return ops.voxel_lovasz_loss(prediction, target, 1.0)[0]


class BoundaryLoss(nn.Module):
    """Distance-transform boundary loss of voxel logits (b, s, c, x, y, z) against uint8 labels (b, s, 1, x, y, z): per frame the
    occupancy probability of every free cell times its distance to the label's nearest occupied cell plus the free probability of
    every occupied label cell times its distance to the prediction's nearest occupied cell, both truncated at `truncate_cells`
    and in units of it, over the label's occupied cells; the mean over the frames with such cells (not in
    the reference).  Label 255 takes no part."""

    def __init__(self, truncate_cells):
        super().__init__()
        if isinstance(truncate_cells, bool) or not isinstance(truncate_cells, int) or truncate_cells < 1:
            raise ValueError(f'truncate_cells must be an integer >= 1, got {truncate_cells!r}')
        self.truncate_cells = truncate_cells

    def forward(self, prediction, target):
        if prediction.dim() != 6 or target.dim() != 6:
            raise ValueError(f'Expected 6-D logits and labels, got {tuple(prediction.shape)} and {tuple(target.shape)}')
        return ops.voxel_boundary_loss(prediction, target, self.truncate_cells, 1.0)[0]


class RenderedDepthLoss(nn.Module):
    """Rendered first-hit depth loss of voxel logits (b, s, c, x, y, z) against uint8 labels (b, s, 1, x, y, z) along the rays of
    one table (R, 7) float32 in grid units, on the device of the logits: the mean over frames and valid rays of |D - t*|, D the
    expected first-hit depth under the head's occupancy probabilities, t* the label's first hit or the exit (DESIGN.md section 12;
    not in the reference).  `n_valid` = the table's valid rays on this grid (voxel_view.valid_rays); counted here when absent."""

    def __init__(self, rays, n_valid=None):
        super().__init__()
        self.rays, self.n_valid = rays, n_valid

    def forward(self, prediction, target):
        if prediction.dim() != 6 or target.dim() != 6:
            raise ValueError(f'Expected 6-D logits and labels, got {tuple(prediction.shape)} and {tuple(target.shape)}')
        n = self.n_valid
        if n is None:
            from muvo_amd.voxel_view import valid_rays
            n = int(valid_rays(self.rays.cpu().numpy(), *prediction.shape[3:]).sum())
        return ops.voxel_render_loss(prediction, target, self.rays, n, 1.0)[0]


class RenderedClassLoss(nn.Module):
    """Rendered first-hit class loss of voxel logits (b, s, c, x, y, z) against uint8 labels (b, s, 1, x, y, z) along the rays of
    one table (R, 7) float32 in grid units, on the device of the logits: the mean over frames and valid rays of
    -log((S_y + 2^-10) / (1 + 2^-10)), S_y the probability that the first occupied cell of the ray has the class y of the label's
    first hit (y = 0: that the ray leaves the grid unhit) under the head's class probabilities (not in the
    reference).  `n_valid` = the table's valid rays on this grid (voxel_view.valid_rays); counted here when absent."""

    def __init__(self, rays, n_valid=None):
        super().__init__()
        self.rays, self.n_valid = rays, n_valid

    def forward(self, prediction, target):
        if prediction.dim() != 6 or target.dim() != 6:
            raise ValueError(f'Expected 6-D logits and labels, got {tuple(prediction.shape)} and {tuple(target.shape)}')
        n = self.n_valid
        if n is None:
            from muvo_amd.voxel_view import valid_rays
            n = int(valid_rays(self.rays.cpu().numpy(), *prediction.shape[3:]).sum())
        return ops.voxel_render_class_loss(prediction, target, self.rays, n, 1.0)[0]


class CDLoss(nn.Module):
    """muvo/losses.py:352-367: Chamfer distance between point clouds (b, s, n, 3), mean over the points of both directions and
    over the frames.  The kernels read channel-planar points, so this drop-in form makes that view (one transposed copy);
    `WorldModelTrainer.compute_loss` hands the head's planar tensors to ops.chamfer_loss directly."""

    def __init__(self, reducer=torch.mean):
        super().__init__()
        if reducer is not torch.mean:
            raise NotImplementedError('the kernels implement reducer = torch.mean (the reference default, losses.py:353)')
        self.reducer = reducer

    def forward(self, prediction, target):
        b, s, n, d = prediction.shape
        if d != 3 or target.shape != prediction.shape:
            raise ValueError(f'Expected (b, s, n, 3) point clouds of equal shape, got {tuple(prediction.shape)} and {tuple(target.shape)}')
        p = prediction.float().permute(0, 1, 3, 2).reshape(b, s, 3, 1, n)
        t = target.float().permute(0, 1, 3, 2).reshape(b, s, 3, 1, n)
        return ops.chamfer_loss(p, t, 1.0)[0]


class SegmentationLoss(nn.Module):
    """muvo/losses.py:9-50: per-pixel (optionally class-weighted) cross entropy on the HIP kernel, then the mean of the
    top-k hardest pixels of every frame (k = int(ratio * h * w)) or of all pixels.  The top-k selection itself is
    torch.topk on the per-pixel loss (a selection, no arithmetic); its gradient flows back into the kernel's backward."""

    def __init__(self, use_top_k=False, top_k_ratio=1.0, use_weights=False, poly_one=False, poly_one_coefficient=0.0, is_bev=True):
        super().__init__()
        if poly_one:
            raise NotImplementedError('poly-1 is never enabled by the reference trainer (trainer.py:132-161)')
        self.use_top_k, self.top_k_ratio, self.use_weights = use_top_k, top_k_ratio, use_weights
        self.weights = (SEMANTIC_SEG_WEIGHTS if is_bev else VOXEL_SEG_WEIGHTS) if use_weights else None

    def forward(self, prediction, target):
        b, s, c, h, w = prediction.shape
        cw = torch.tensor(self.weights, dtype=torch.float32, device=prediction.device) if self.weights is not None else None
        loss = ops.seg_ce_pixel_loss(prediction.reshape(b * s, c, h, w), target.reshape(b * s, h, w), cw).view(b, s, -1)
        if self.use_top_k:
            k = int(self.top_k_ratio * loss.shape[2])
            loss = loss.topk(k, dim=-1)[0]
        return torch.mean(loss)


class _SSIMMeanFn(torch.autograd.Function):
    """mean over frames of the per-frame mean SSIM map (SSIMLoss.forward, losses.py:341-348), differentiable in the prediction."""

    @staticmethod
    def forward(ctx, prediction, target, win, c1, c2):
        n, c, h, w = prediction.shape
        p, t = prediction.contiguous(), target.float().contiguous()
        oh, ow = h - 10, w - 10
        sums = torch.zeros(n, dtype=torch.float64, device=p.device)
        maps = torch.empty(3, n, c, oh, ow, device=p.device, dtype=torch.float32)
        ops._ck(ops.lib().muvo_ssim_maps(ops._f(p), ops._f(t), ops._f(win), ops._p(sums), ops._f(maps[0]), ops._f(maps[1]), ops._f(maps[2]),
                                        n, c, h, w, ops._fl(c1), ops._fl(c2), ops._st()))
        ctx.save_for_backward(p, t, win, maps)
        return (sums / (c * oh * ow)).mean().float()

    @staticmethod
    def backward(ctx, g):
        p, t, win, maps = ctx.saved_tensors
        n, c, h, w = p.shape
        dp = torch.empty_like(p)
        scale = float(g) / (n * c * (h - 10) * (w - 10))
        ops._ck(ops.lib().muvo_ssim_bwd(ops._f(p), ops._f(t), ops._f(win), ops._f(maps[0]), ops._f(maps[1]), ops._f(maps[2]), ops._f(dp), n, c,
                                       h, w, ops._fl(scale), ops._st()))
        return dp, None, None, None, None


class SSIMLoss(nn.Module):
    """muvo/losses.py:292-348 (returns the mean SSIM; the trainer uses 1 - it, trainer.py:312-318)."""

    def __init__(self, channel=1, window_size=11, sigma=1.5, L=1, non_negative=False):
        super().__init__()
        if window_size != 11 or non_negative:
            raise NotImplementedError('the kernels implement the reference configuration (window 11, non_negative=False)')
        from .metrics import _gauss_window
        self.channel, self.C1, self.C2 = channel, (0.01 * L) ** 2, (0.03 * L) ** 2
        self.register_buffer('window2d', _gauss_window(window_size, sigma), persistent=False)

    def forward(self, prediction, target):
        b, s, c, h, w = prediction.shape
        win = self.window2d.to(prediction.device)
        return _SSIMMeanFn.apply(prediction.reshape(b * s, c, h, w).float(), target.reshape(b * s, c, h, w), win, self.C1, self.C2)
