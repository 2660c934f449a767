"""WorldModelTrainer — drop-in for muvo/trainer.py's LightningModule on the MI355X-native step.

Same constructor `(hparams, path_to_conf_file=None, pretrained_path=None)`, attributes (`cfg`, `rf`, `fh`,
`preprocess`, `model`) and methods (`forward`, `compute_loss`, `shared_step(mode='train')`, `training_step`,
`configure_optimizers`, `load_pretrained_weights`) as trainer.py:26-231,251-402,511-513,1022-1073.  If
`lightning` is importable the class derives from `pl.LightningModule`, otherwise from `torch.nn.Module` with
the same hooks so the build's own loop (bench.py / train.py / predict.py) can drive it.  The evaluation half (`validation_step`,
`test_step`, `log_metrics`, `on_validation_epoch_end`, `on_test_epoch_end`; trainer.py:404-567,1075-1095) is here too; the three
torchmetrics IoU metrics are muvo_amd.metrics.JaccardIndex.  `visualise` (trainer.py:569-957) renders the picture
grids on the device (muvo_amd/visualise.py) and hands them to `panel_writer`; while that is None - the default - nothing is drawn."""
import os

import numpy as np
import torch

from muvo_amd import ops
from muvo_amd.config import (get_cfg, lidar_cd, voxel_boundary, voxel_boundary_cells, voxel_lovasz, voxel_render, voxel_render_class,
                             voxel_aggregate, voxel_visibility)
from muvo_amd.models.mile import Mile
from muvo_amd.models.preprocess import PreProcess
from muvo_amd.optim import FusedAdamW
from muvo_amd.param_store import ParamStore

try:  # optional: Lightning is not a dependency of the hot path
    import lightning.pytorch as pl
    _Base = pl.LightningModule
except Exception:  # pragma: no cover
    pl = None
    _Base = torch.nn.Module


_DDP_MSG = ('muvo_amd.WorldModelTrainer exchanges its gradients itself (segmented RCCL all-reduce on a side stream, '
            'muvo_amd/parallel.py): run one process per GPU with torch.distributed initialised and do NOT wrap the '
            'module in DistributedDataParallel (Lightning: use a single-device strategy per process, INTEGRATION.md §5)')


def _refuse_ddp(module, args):
    tr = getattr(module, '_trainer', None) if pl is not None else None
    strategy = getattr(tr, 'strategy', None)
    if strategy is not None and isinstance(getattr(strategy, 'model', None), torch.nn.parallel.DistributedDataParallel):
        raise RuntimeError(_DDP_MSG)


VOXEL_LABEL = ('Background', 'Occupancy')          # the names of the reference's voxel class table (constants.py VOXEL_LABEL)
BEV_CLASS_NAMES = ('Background', 'Road', 'Lane marking', 'Vehicle', 'Pedestrian', 'Green light', 'Yellow light',
                   'Red light and stop sign')       # trainer.py:520-521
# (metric key, config node, its class-count field, tag in the logged names, class names the per-class scores are zipped with)
IOU_HEADS = (('iou', 'SEMANTIC_SEG', 'N_CHANNELS', 'bev', BEV_CLASS_NAMES),
             ('pcd_iou', 'LIDAR_SEG', 'N_CLASSES', 'lidar', VOXEL_LABEL),
             ('image_iou', 'SEMANTIC_IMAGE', 'N_CLASSES', 'camera', VOXEL_LABEL))


def _iou_names(cfg, prefix, head):
    key, node, field, tag, class_names = head
    if not cfg[node].ENABLED:
        return []
    return [f'{prefix}_{tag}_iou_{name}' for name in class_names[:cfg[node][field]]] + [f'{prefix}_{tag}_mean_iou']


def metric_names(cfg, prefix):
    """Every name log_metrics sends for one non-empty metric set, in the reference's order (trainer.py:525-567): the IoU
    names of the segmentation heads, which travel on the logger channel (log_scalar), interleaved with those of
    metric_log_names.  The zip with the class-name table stops at the shorter side, like the reference's."""
    names = _iou_names(cfg, prefix, IOU_HEADS[0])
    if cfg.EVAL.RGB_SUPERVISION:
        names += [f'{prefix}_ssim', f'{prefix}_psnr']
    if cfg.LIDAR_RE.ENABLED:
        names.append(f'{prefix}_chamfer_distance')
    names += _iou_names(cfg, prefix, IOU_HEADS[1]) + _iou_names(cfg, prefix, IOU_HEADS[2])
    if cfg.VOXEL_SEG.ENABLED:
        names += [f'{prefix}_Voxel_{name}_SemIoU' for name in VOXEL_LABEL[:cfg.VOXEL_SEG.N_CLASSES]]
        names += [f'{prefix}_Voxel_mIoU', f'{prefix}_Voxel_IoU', f'{prefix}_Voxel_Precision', f'{prefix}_Voxel_Recall']
        if voxel_visibility(cfg)[0]:       # extension (config.py: VOXEL_SEG.VISIBILITY), absent = off: no such name
            names.append(f'{prefix}_Voxel_Unknown_Share')
        if voxel_aggregate(cfg)[0]:        # extension (config.py: VOXEL_SEG.AGGREGATE), absent = off: no such names
            names += [f'{prefix}_Voxel_Filled_Share', f'{prefix}_Voxel_Unknown_Share_Aggregated']
    return names


def metric_log_names(cfg, prefix):
    """The names log_metrics sends through `self.log` for one non-empty metric set, in order (trainer.py:532-567)."""
    names = []
    if cfg.EVAL.RGB_SUPERVISION:
        names += [f'{prefix}_ssim', f'{prefix}_psnr']
    if cfg.LIDAR_RE.ENABLED:
        names.append(f'{prefix}_chamfer_distance')
    if cfg.VOXEL_SEG.ENABLED:
        names += [f'{prefix}_Voxel_{name}_SemIoU' for name in VOXEL_LABEL[:cfg.VOXEL_SEG.N_CLASSES]]
        names += [f'{prefix}_Voxel_mIoU', f'{prefix}_Voxel_IoU', f'{prefix}_Voxel_Precision', f'{prefix}_Voxel_Recall']
        if voxel_visibility(cfg)[0]:       # extension (config.py: VOXEL_SEG.VISIBILITY), absent = off: no such name
            names.append(f'{prefix}_Voxel_Unknown_Share')
        if voxel_aggregate(cfg)[0]:        # extension (config.py: VOXEL_SEG.AGGREGATE), absent = off: no such names
            names += [f'{prefix}_Voxel_Filled_Share', f'{prefix}_Voxel_Unknown_Share_Aggregated']
    return names


def voxel_target(cfg, batch, f):
    """The labels of the dense voxel terms and the SSC counts at scale f: `voxel_visible_label_{f}` with VOXEL_SEG.VISIBILITY on
    (unobserved free cells are 255, which those kernels ignore), `voxel_label_{f}` otherwise.  The ray-based users - the rendered
    depth and class losses, RayIoU, the panels, the sim export - always read `voxel_label_{f}`: a 255 would be an occupied cell to them."""
    return batch[f'voxel_visible_label_{f}' if voxel_visibility(cfg)[0] else f'voxel_label_{f}']


def metric_heads_left_out(cfg):
    """Enabled heads whose metric is an IoU (torchmetrics.JaccardIndex in the reference, muvo_amd.metrics.JaccardIndex here,
    trainer.py:525-554): their scores travel on the logger channel (`log_scalar`), not through `self.log`, so their names are
    in metric_names and not in metric_log_names."""
    heads = (('SEMANTIC_SEG', 'bev_iou'), ('LIDAR_SEG', 'lidar_iou'), ('SEMANTIC_IMAGE', 'camera_iou'))
    return [name for key, name in heads if cfg[key].ENABLED]


class WorldModelTrainer(_Base):
    def __init__(self, hparams, path_to_conf_file=None, pretrained_path=None, device=None):
        super().__init__()
        if pl is not None:
            self.save_hyperparameters()
        self.cfg = get_cfg(cfg_dict=hparams)
        if path_to_conf_file:
            self.cfg.merge_from_file(path_to_conf_file)
        if pretrained_path:
            self.cfg.PRETRAINED.PATH = pretrained_path
        self.vis_step = -1
        self.rf = self.cfg.RECEPTIVE_FIELD
        self.fh = self.cfg.FUTURE_HORIZON
        ops.lib()  # fail loudly, before building anything, if the HIP library is missing
        self.preprocess = PreProcess(self.cfg)
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None
        if device is None:
            raise RuntimeError('muvo_amd needs a GPU (gfx950): no CUDA/HIP device visible and there is no CPU path')
        with torch.device(device):
            self.model = Mile(self.cfg)
        self.load_pretrained_weights()
        self.store = None
        self._optimizer = None
        self._reducer = None
        self._global_step = 0          # plain-loop counterpart of LightningModule.global_step
        self.log_fn = None             # plain loop: callable(name, value) receiving what Lightning's self.log would
        self.logged = {}
        self.on_confusion = None       # callable(name, (C, C) host int64 matrix): the IoU heads' counts, handed over by log_metrics
        self.accumulate_now = False    # plain loop: True while a non-final micro-batch of gradient accumulation runs
        self.panel_writer = None       # object with add_images / add_video (muvo_amd.visualise.PanelWriter): None = no panels
        self.traj_panels = False       # with a writer and LIDAR_RE: also `_traj` (muvo_amd/odometry.py, ICP between lidar frames)
        self.traj_options = {}         # threshold / source_stride / max_iteration / search of that ICP (default: 5 m, 1, 2000, brute)
        self.flow_panels = False       # with a writer and EVAL.RGB_SUPERVISION: also `_flow` (muvo_amd/flow.py, dense optical flow)
        self.voxel_panels = False      # with a writer and VOXEL_SEG: also `_voxel` (muvo_amd/voxel_view.py, ray-cast 3-D view)
        self.voxel_options = {}        # size of that panel's tiles (default 256)
        self.inst_panels = False       # with a writer and SEMANTIC_SEG: also `_inst` (muvo_amd/bev_instances.py, decoded BEV instances)
        self.inst_options = {}         # decode options of that panel (threshold, radius, max_centres, thing_classes)
        self.uncert_panels = False     # with a writer and VOXEL_SEG: also `_uncert` (muvo_amd/calibration.py, entropy and mutual information)
        # evaluation metrics per validation / test dataloader (trainer.py:51-55,100-129,191-197); created on first use
        # because they hold device accumulators
        self.metrics_vals = [{}, {}, {}]
        self.metrics_vals_imagine = [{}, {}, {}]
        self.metrics_tests = [{}, {}, {}]
        self.metrics_tests_imagine = [{}, {}, {}]

    # ------------------------------------------------------------------ weights
    def load_pretrained_weights(self):
        path = self.cfg.PRETRAINED.PATH
        if path:
            if os.path.isfile(path):
                checkpoint = torch.load(path, map_location='cpu')['state_dict']
                checkpoint = {key[6:]: value for key, value in checkpoint.items() if key[:5] == 'model'}
                self.model.load_state_dict(checkpoint, strict=True)
                print(f'Loaded weights from: {path}')
            else:
                raise FileExistsError(path)

    # ------------------------------------------------------------------ forward / losses
    def forward(self, batch, deployment=False, noise=None, use_prior=None):
        ops.repack_all()           # one launch refreshes every packed weight copy made stale by the optimizer step
        batch = self.preprocess(batch)
        output, state_dict = self.model.forward(batch, deployment=deployment, noise=noise, use_prior=use_prior)
        return output, state_dict

    def deployment_forward(self, batch, is_dreaming):
        """trainer.py:218-221"""
        ops.repack_all()
        batch = self.preprocess(batch)
        return self.model.deployment_forward(batch, is_dreaming)

    def shared_step(self, batch, mode='train', predict_action=False, noise=None, use_prior=None):
        """trainer.py:223-249.  mode='train': reconstruction of the whole sequence.  Otherwise: reconstruct the first
        RECEPTIVE_FIELD frames, then imagine FUTURE_HORIZON steps from the last posterior state and score them against the
        remaining frames.  noise (b, rf + N_SAMPLES*fh, 2, S) / use_prior (rf,) make the RNG explicit: [:, t < rf] feed the
        observe steps, [:, rf + k*fh + t, 0] step t of imagined sample k."""
        if mode == 'train':
            try:
                output, state_dict = self.forward(batch, noise=noise, use_prior=use_prior)
                losses = self.compute_loss(batch, output)
            except BaseException:
                ops.reset_accumulators()      # zero-between-uses buffers may hold partial sums of the interrupted step
                raise
            return losses, output, [], []
        rf, fh = self.rf, self.fh
        batch = self.preprocess(batch)
        # (b, s, ...) tensors are cut in time; `voxel_aggregate_counts` (3,) has no time axis and stays whole
        batch_rf = {k: v[:, :rf].contiguous() if v.dim() >= 2 else v for k, v in batch.items()}
        batch_fh = {k: v[:, rf:].contiguous() if v.dim() >= 2 else v for k, v in batch.items()}
        output, state_dict = self.model.forward(batch_rf, deployment=False, noise=None if noise is None else noise[:, :rf],
                                                use_prior=None if use_prior is None else list(use_prior[:rf]))
        losses = self.compute_loss(batch_rf, output)
        post = state_dict['posterior']
        state_imagine = {'hidden_state': post['hidden_state'][:, -1], 'sample': post['sample'][:, -1],
                         'throttle_brake': batch_fh['throttle_brake'], 'steering': batch_fh['steering']}
        output_imagines, losses_imagines = [], []
        for k in range(self.cfg.PREDICTION.N_SAMPLES):
            # explicit noise layout: (b, rf + N_SAMPLES * fh, 2, S); sample k of the roll-out uses rows rf + k*fh ...
            nz = None if noise is None else noise[:, rf + k * fh:rf + (k + 1) * fh, 0].contiguous()
            out_i = self.model.imagine(state_imagine, predict_action=predict_action, future_horizon=fh, noise=nz)
            output_imagines.append(out_i)
            losses_imagines.append(self.compute_loss(batch_fh, out_i))
        return losses, output, losses_imagines, output_imagines

    def _metric_set(self, metrics):
        """trainer.py:73-197: the metrics of the enabled heads (base_1d: ssim, psnr, cd, ssc; iou, pcd_iou, image_iou with the
        bird's-eye-view, lidar and camera segmentation heads)."""
        if not metrics:
            from .metrics import CDMetric, JaccardIndex, PSNRMetric, SSCMetrics, SSIMMetric
            for key, node, field, _, _ in IOU_HEADS:
                if self.cfg[node].ENABLED:
                    metrics[key] = JaccardIndex(task='multiclass', num_classes=self.cfg[node][field], average='none')
            if self.cfg.EVAL.RGB_SUPERVISION:
                metrics['ssim'], metrics['psnr'] = SSIMMetric(channel=3), PSNRMetric(max_pixel_val=1.0)
            if self.cfg.LIDAR_RE.ENABLED:
                metrics['cd'] = CDMetric()
            if self.cfg.VOXEL_SEG.ENABLED:
                metrics['ssc'] = SSCMetrics(self.cfg.VOXEL_SEG.N_CLASSES)
                if voxel_visibility(self.cfg)[0]:
                    from .metrics import VoxelUnknownShare
                    metrics['unknown'] = VoxelUnknownShare()
                if voxel_aggregate(self.cfg)[0]:
                    from .metrics import VoxelFilledShare
                    metrics['filled'] = VoxelFilledShare()
        return metrics

    def add_metrics(self, metrics, batch, output, cd_index=None):
        """trainer.py:426-480.  cd_index: the 10000-point subset of the Chamfer metric; the reference draws it with
        np.random.randint (trainer.py:455), pass it explicitly for reproducible numbers.  The IoU metrics get the heads' logits:
        the argmax of trainer.py:429,466,474 is part of the counting kernel, and neither side goes to the host."""
        metrics = self._metric_set(metrics)
        if self.cfg.SEMANTIC_SEG.ENABLED:
            metrics['iou'](output['bev_segmentation_1'].detach().flatten(0, 1), batch['birdview_label'])
        if self.cfg.EVAL.RGB_SUPERVISION:
            metrics['ssim'].add_batch(prediction=output['rgb_1'].detach(), target=batch['rgb_label_1'])
            metrics['psnr'].add_batch(prediction=output['rgb_1'].detach(), target=batch['rgb_label_1'])
        if self.cfg.LIDAR_RE.ENABLED:
            lidar_target = batch['range_view_label_1']
            lidar_pred = output['lidar_reconstruction_1'].detach()
            pcd_target = lidar_target.detach().permute(0, 1, 3, 4, 2).flatten(2, 3).flatten(0, 1) * self.cfg.LIDAR_RE.SCALE
            pcd_pred = lidar_pred.permute(0, 1, 3, 4, 2).flatten(2, 3).flatten(0, 1) * self.cfg.LIDAR_RE.SCALE
            if cd_index is None:
                cd_index = np.random.randint(0, pcd_target.size(-2), 10000)
            index = torch.as_tensor(cd_index, device=pcd_pred.device).long()
            metrics['cd'].add_batch(pcd_pred[:, index, :-1], pcd_target[:, index, :-1])
        if self.cfg.LIDAR_SEG.ENABLED:
            metrics['pcd_iou'](output['lidar_segmentation_1'].detach().flatten(0, 1), batch['range_view_seg_label_1'])
        if self.cfg.SEMANTIC_IMAGE.ENABLED:
            metrics['image_iou'](output['semantic_image_1'].detach().flatten(0, 1), batch['semantic_image_label_1'])
        if self.cfg.VOXEL_SEG.ENABLED:
            self.compute_ssc_metrics(batch, output, metrics['ssc'])
            if 'unknown' in metrics:
                from muvo_amd.voxel_view import visibility_table
                label = batch['voxel_label_1']
                grid = label.to(torch.uint8).reshape(-1, *label.shape[-3:])
                metrics['unknown'].add_batch(grid, visibility_table(self.cfg, 1, tuple(grid.shape[1:]), grid.device))
            if 'filled' in metrics:          # the counts of the WHOLE batch (a frame is filled from both sides of the rf / fh split)
                metrics['filled'].add_batch(batch['voxel_aggregate_counts'], batch.get('voxel_aggregate_cells', batch['voxel_label_1'].numel()))

    def compute_ssc_metrics(self, batch, output, metric):
        """trainer.py:482-490; the argmax over the class logits happens inside the counting kernel."""
        y_true = voxel_target(self.cfg, batch, 1)
        y_pred = output['voxel_1'].detach()
        b, s, c, x, y, z = y_pred.shape
        metric.add_batch(y_pred.reshape(b * s, c, x, y, z), y_true.reshape(b * s, x, y, z))

    def _eval_step(self, batch, mode, metrics, metrics_imagine, noise, use_prior, cd_index):
        """The body validation_step and test_step share (trainer.py:404-417,1079-1092): train-mode BatchNorm, transformer
        nn.Dropout modules off (the functional attention dropout of nn.MultiheadAttention stays on), no_grad;
        then the reconstruction metrics on the observed frames and the imagination metrics on the future frames."""
        self.train()
        layers = list(self.model.transformer_encoder.layers)
        saved = [getattr(layer, 'module_dropout_off', False) for layer in layers]
        for layer in layers:
            layer.module_dropout_off = True
        try:
            with torch.no_grad():
                loss, output, loss_imagines, output_imagines = self.shared_step(batch, mode=mode, predict_action=False,
                                                                                noise=noise, use_prior=use_prior)
        finally:
            for layer, v in zip(layers, saved):
                layer.module_dropout_off = v
        batch_rf = {key: value[:, :self.rf] if value.dim() >= 2 else value for key, value in batch.items() if torch.is_tensor(value)}
        batch_fh = {key: value[:, self.rf:] if value.dim() >= 2 else value for key, value in batch.items() if torch.is_tensor(value)}
        if 'voxel_aggregate_counts' in batch:       # (3,): no time axis to cut; both sets count the whole batch and its cells
            batch_rf['voxel_aggregate_cells'] = batch_fh['voxel_aggregate_cells'] = batch['voxel_label_1'].numel()
        self.add_metrics(metrics, batch_rf, output, cd_index)
        for output_imagine in output_imagines:
            self.add_metrics(metrics_imagine, batch_fh, output_imagine, cd_index)
        return loss, output, loss_imagines, output_imagines

    def validation_step(self, batch, batch_idx=0, dataloader_idx=0, noise=None, use_prior=None, cd_index=None):
        """trainer.py:404-424; the logging / visualisation hook runs while `panel_writer` is set."""
        loss, output, loss_imagines, output_imagines = self._eval_step(
            batch, 'val', self.metrics_vals[dataloader_idx], self.metrics_vals_imagine[dataloader_idx], noise, use_prior, cd_index)
        if self.panel_writer is not None:
            self.logging_and_visualisation(batch, output, output_imagines, loss, loss_imagines, batch_idx, prefix=f'val{dataloader_idx}')
        out = {f'val{dataloader_idx}_loss': self.loss_reducing(loss),
               f'val{dataloader_idx}_loss_imagine': sum(self.loss_reducing(li) for li in loss_imagines) / len(loss_imagines)}
        return out, loss, output, loss_imagines, output_imagines

    def test_step(self, batch, batch_idx=0, dataloader_idx=0, noise=None, use_prior=None, cd_index=None):
        """trainer.py:1079-1095: the evaluation step feeding `metrics_tests` / `metrics_tests_imagine`; returns (output,
        output_imagines).  While `panel_writer` is set every batch is drawn (prefix `pred{dataloader_idx}`)."""
        _, output, _, output_imagines = self._eval_step(
            batch, 'test', self.metrics_tests[dataloader_idx], self.metrics_tests_imagine[dataloader_idx], noise, use_prior, cd_index)
        if self.panel_writer is not None:
            self.visualise(batch, output, output_imagines, batch_idx, prefix=f'pred{dataloader_idx}')
        return output, output_imagines

    def log_metrics(self, metrics_list, metrics_type):
        """trainer.py:519-567: every non-empty metric set of `metrics_list` goes out under `{metrics_type}{idx}_...`
        (metric_names) and is reset.  The per-class and mean IoU of the bird's-eye-view, lidar and camera heads go through
        `log_scalar` (the reference's `self.logger.experiment.add_scalar`), everything else through `self.log`
        (metric_log_names).  `on_confusion(name, matrix)`, if set, gets each head's (C, C) count matrix - host int64, already
        read for the scores - before the reset."""
        for idx, metrics in enumerate(metrics_list):
            if not metrics:
                continue
            prefix = f'{metrics_type}{idx}'
            self._log_iou(metrics, prefix, IOU_HEADS[0])
            if 'ssim' in metrics:
                self.log(f'{prefix}_ssim', metrics['ssim'].get_stat())
                metrics['ssim'].reset()
                self.log(f'{prefix}_psnr', metrics['psnr'].get_stat())
                metrics['psnr'].reset()
            if 'cd' in metrics:
                self.log(f'{prefix}_chamfer_distance', metrics['cd'].get_stat())
                metrics['cd'].reset()
            self._log_iou(metrics, prefix, IOU_HEADS[1])
            self._log_iou(metrics, prefix, IOU_HEADS[2])
            if 'ssc' in metrics:
                stats = metrics['ssc'].get_stats()
                for class_name, value in zip(VOXEL_LABEL, stats['iou_ssc']):        # stops at the shorter list, like the reference
                    self.log(f'{prefix}_Voxel_{class_name}_SemIoU', value)
                self.log(f'{prefix}_Voxel_mIoU', stats['iou_ssc_mean'])
                self.log(f'{prefix}_Voxel_IoU', stats['iou'])
                self.log(f'{prefix}_Voxel_Precision', stats['precision'])
                self.log(f'{prefix}_Voxel_Recall', stats['recall'])
                metrics['ssc'].reset()
            if 'unknown' in metrics:
                self.log(f'{prefix}_Voxel_Unknown_Share', metrics['unknown'].get_stat())
                metrics['unknown'].reset()
            if 'filled' in metrics:
                filled, unknown = metrics['filled'].get_stat()
                self.log(f'{prefix}_Voxel_Filled_Share', filled)
                self.log(f'{prefix}_Voxel_Unknown_Share_Aggregated', unknown)
                metrics['filled'].reset()

    def _log_iou(self, metrics, prefix, head):
        """trainer.py:525-530,542-554 for one head: per-class scores zipped with the class names, the mean over ALL classes."""
        key, _, _, tag, class_names = head
        if key not in metrics:
            return
        scores, confmat = metrics[key].compute(with_confmat=True)
        for name, value in zip(class_names, scores):
            self.log_scalar(f'{prefix}_{tag}_iou_{name}', value)
        self.log_scalar(f'{prefix}_{tag}_mean_iou', torch.mean(scores))
        if self.on_confusion is not None:
            self.on_confusion(f'{prefix}_{tag}_confusion', confmat)
        metrics[key].reset()

    def log_scalar(self, name, value):
        """The reference's `self.logger.experiment.add_scalar(name, value, global_step=self.global_step)`: under Lightning
        with a logger whose `experiment` has `add_scalar` (TensorBoard) exactly that; otherwise the value goes to
        `self.log_fn(name, value)` if one is set, else into `self.logged`."""
        if pl is not None and getattr(self, '_trainer', None) is not None:
            experiment = getattr(getattr(self, 'logger', None), 'experiment', None)
            if hasattr(experiment, 'add_scalar'):
                experiment.add_scalar(name, value, global_step=self.global_step)
                return
        if torch.is_tensor(value):
            value = value.detach()
        if self.log_fn is not None:
            self.log_fn(name, value)
        else:
            self.logged[name] = value

    def on_validation_epoch_end(self):
        """trainer.py:515-517"""
        self.log_metrics(self.metrics_vals, 'val')
        self.log_metrics(self.metrics_vals_imagine, 'val_imagine')

    def on_test_epoch_end(self):
        """trainer.py:1075-1077"""
        self.log_metrics(self.metrics_tests, 'test')
        self.log_metrics(self.metrics_tests_imagine, 'test_imagine')

    def compute_loss(self, batch, output):
        """The reference's 21 weighted loss terms (trainer.py:251-390), computed by fused kernels."""
        cfg = self.cfg
        losses = {}
        w_act = cfg.LOSSES.WEIGHT_ACTION
        if 'throttle_brake' in output:
            losses['throttle_brake'] = ops.l1_rows_loss(output['throttle_brake'], batch['throttle_brake'], w_act, terms=True)[0]
        if 'steering' in output:
            losses['steering'] = ops.l1_rows_loss(output['steering'], batch['steering'], w_act, terms=True)[0]
        if cfg.MODEL.TRANSITION.ENABLED and 'prior' in output and 'posterior' in output:
            pr, po = output['prior'], output['posterior']
            losses['probabilistic'] = ops.kl_loss(pr['mu'], pr['sigma'], po['mu'], po['sigma'],
                                                  cfg.LOSSES.WEIGHT_PROBABILISTIC, cfg.LOSSES.KL_BALANCING_ALPHA, terms=True)[0]
        if cfg.SEMANTIC_SEG.ENABLED:              # trainer.py:266-291
            crit = self._seg_loss('bev', cfg.SEMANTIC_SEG, is_bev=True)
            ign = float(cfg.INSTANCE_SEG.IGNORE_INDEX)
            for f in (1, 2, 4):
                d = 1 / f
                losses[f'bev_segmentation_{f}'] = crit(output[f'bev_segmentation_{f}'], batch[f'birdview_label_{f}']) \
                    * (d * cfg.LOSSES.WEIGHT_SEGMENTATION)
                wc = d * cfg.LOSSES.WEIGHT_INSTANCE * cfg.INSTANCE_SEG.CENTER_LOSS_WEIGHT
                losses[f'bev_center_{f}'] = ops.spatial_losses(output[f'bev_instance_center_{f}'], batch[f'center_label_{f}'],
                                                               [(0, 1, 2, wc)])[0]
                wo = cfg.LOSSES.WEIGHT_INSTANCE * cfg.INSTANCE_SEG.OFFSET_LOSS_WEIGHT   # offsets are discounted in the labels
                losses[f'bev_offset_{f}'] = ops.spatial_losses(output[f'bev_instance_offset_{f}'], batch[f'offset_label_{f}'],
                                                               [(0, 2, 1, wo)], ign)[0]
        if cfg.EVAL.RGB_SUPERVISION:
            for f in (1, 2, 4):
                w = 0.1 * (1 / f)  # rgb_weight literal 0.1 (trainer.py:296)
                pred = output[f'rgb_{f}']
                losses[f'rgb_{f}'] = ops.spatial_losses(pred, batch[f'rgb_label_{f}'], [(0, pred.shape[2], 1, w)], terms=True)[0]
                if cfg.LOSSES.RGB_INSTANCE:       # trainer.py:303-321: + 0.5 x the same L1 over the vehicle / pedestrian pixels
                    losses[f'rgb_{f}'] = losses[f'rgb_{f}'] + ops.spatial_losses(
                        pred, batch[f'rgb_label_{f}'], [(0, pred.shape[2], 1, 0.5 * w)], mask=batch[f'image_instance_mask_{f}'])[0]
                if cfg.LOSSES.SSIM:               # trainer.py:312-318: 0.6 * (1 - mean SSIM), same rgb weight and discount
                    if '_ssim_loss' not in self.__dict__:
                        from .losses import SSIMLoss
                        self.__dict__['_ssim_loss'] = SSIMLoss(channel=3)
                    losses[f'ssim_{f}'] = (1 - self.__dict__['_ssim_loss'](pred, batch[f'rgb_label_{f}'])) * (w * 0.6)
        if cfg.LIDAR_RE.ENABLED:
            for f in (1, 2, 4):
                w = (1 / f) * cfg.LOSSES.WEIGHT_LIDAR_RE
                pred = output[f'lidar_reconstruction_{f}']
                c = pred.shape[2]
                both = ops.spatial_losses(pred, batch[f'range_view_label_{f}'], [(0, 3, 2, w), (c - 1, c, 1, w)], terms=True)
                losses[f'lidar_re_{f}'] = both[0]
                losses[f'lidar_depth_{f}'] = both[1]
        # config-off heads of base_1d (trainer.py:338-365)
        if cfg.LIDAR_SEG.ENABLED:
            crit = self._seg_loss('lidar', cfg.LIDAR_SEG)
            for f in (1, 2, 4):
                losses[f'lidar_seg_{f}'] = crit(output[f'lidar_segmentation_{f}'], batch[f'range_view_seg_label_{f}']) \
                    * ((1 / f) * cfg.LOSSES.WEIGHT_LIDAR_SEG)
        if cfg.SEMANTIC_IMAGE.ENABLED:
            crit = self._seg_loss('image', cfg.SEMANTIC_IMAGE)
            for f in (1, 2, 4):
                losses[f'semantic_image_{f}'] = crit(output[f'semantic_image_{f}'], batch[f'semantic_image_label_{f}']) \
                    * ((1 / f) * cfg.LOSSES.WEIGHT_SEM_IMAGE)
        if cfg.DEPTH.ENABLED:
            for f in (1, 2, 4):
                w = (1 / f) * cfg.LOSSES.WEIGHT_DEPTH
                losses[f'depth_{f}'] = ops.spatial_losses(output[f'depth_{f}'], batch[f'depth_label_{f}'], [(0, 1, 1, w)])[0]
        if cfg.VOXEL_SEG.ENABLED:
            for f in (1, 2, 4):
                w = (1 / f) * cfg.LOSSES.WEIGHT_VOXEL
                vs = cfg.VOXEL_SEG
                cw = None
                if vs.USE_WEIGHTS:                # constants.py:39 through VoxelLoss(use_weights) (losses.py:155-165)
                    from .losses import VOXEL_SEG_WEIGHTS
                    logits_f = output[f'voxel_{f}']
                    if len(VOXEL_SEG_WEIGHTS) != logits_f.shape[2]:      # F.cross_entropy of the reference raises here as well
                        raise RuntimeError(f'VOXEL_SEG.USE_WEIGHTS: {len(VOXEL_SEG_WEIGHTS)} class weights (constants.py:39) for '
                                           f'{logits_f.shape[2]} voxel classes')
                    cache = self.__dict__.setdefault('_voxel_class_weights', {})     # one H2D copy per device, not three per step
                    cw = cache.get(logits_f.device)
                    if cw is None:
                        cw = cache[logits_f.device] = torch.tensor(VOXEL_SEG_WEIGHTS, dtype=torch.float32, device=logits_f.device)
                # (USE_TOP_K replaces the cross-entropy term: the fused kernel then only delivers the two scaling terms)
                three = ops.voxel_losses(output[f'voxel_{f}'], voxel_target(cfg, batch, f), w, cw, terms=True)
                if vs.USE_TOP_K:                  # losses.py:179-184: the k hardest voxels of every frame
                    from .losses import VoxelLoss
                    crit = self.__dict__.setdefault('_voxel_topk', VoxelLoss(True, vs.TOP_K_RATIO, vs.USE_WEIGHTS))
                    losses[f'voxel_{f}'] = crit(output[f'voxel_{f}'], batch[f'voxel_label_{f}']) * w
                else:
                    losses[f'voxel_{f}'] = three[0]
                losses[f'sem_scal_{f}'] = three[1]
                losses[f'geo_scal_{f}'] = three[2]
        # the Chamfer distance of the lidar head (CDLoss, losses.py:352-367; the reference constructs it only in a comment,
        # trainer.py:116): after the reference's terms, so that their order - and the order of the total's sum - stays as it is
        w_cd, cd_factors = lidar_cd(cfg)
        if w_cd > 0:                              # extension (config.py: LOSSES.LIDAR_CD), absent = off: no term, no launch
            for f in cd_factors:                  # x, y, z = channels 0..2 of both tensors, in the scaled units of lidar_re_*
                losses[f'lidar_cd_{f}'] = ops.chamfer_loss(output[f'lidar_reconstruction_{f}'], batch[f'range_view_label_{f}'],
                                                           w_cd * (1 / f), terms=True)[0]
        # the Lovasz-softmax loss of the voxel head (extension, config.py: LOSSES.VOXEL_LOVASZ; absent = off: no term, no launch),
        # last for the same reason
        w_lv, lv_factors = voxel_lovasz(cfg)
        if w_lv > 0:
            for f in lv_factors:
                losses[f'voxel_lovasz_{f}'] = ops.voxel_lovasz_loss(output[f'voxel_{f}'], voxel_target(cfg, batch, f), w_lv * (1 / f),
                                                                    terms=True)[0]
        # the rendered first-hit depth loss of the voxel head along the lidar's rays (extension, config.py: LOSSES.VOXEL_RENDER;
        # absent = off: no term, no launch, no table), last for the same reason.  In the scaled depth units of lidar_depth_f:
        # grid cells of scale f are VOXEL.RESOLUTION f metres
        w_rd, rd_factors, rd_stride = voxel_render(cfg)
        if w_rd > 0:
            from muvo_amd.voxel_view import render_table
            for f in rd_factors:
                pred = output[f'voxel_{f}']
                rays, n_valid = render_table(cfg, f, rd_stride, tuple(pred.shape[3:]), pred.device)
                losses[f'voxel_render_{f}'] = ops.voxel_render_loss(pred, batch[f'voxel_label_{f}'], rays, n_valid,
                                                                    w_rd * (1 / f) * (cfg.VOXEL.RESOLUTION * f / cfg.LIDAR_RE.SCALE),
                                                                    terms=True)[0]
        # the rendered first-hit class loss along the same rays (extension, config.py: LOSSES.VOXEL_RENDER_CLASS; absent = off: no
        # term, no launch, no table), last for the same reason; the table is the depth term's when both keys use one stride, and
        # like it the loss reads the unmasked labels
        w_rc, rc_factors, rc_stride = voxel_render_class(cfg)
        if w_rc > 0:
            from muvo_amd.voxel_view import render_table
            for f in rc_factors:
                pred = output[f'voxel_{f}']
                rays, n_valid = render_table(cfg, f, rc_stride, tuple(pred.shape[3:]), pred.device)
                losses[f'voxel_render_class_{f}'] = ops.voxel_render_class_loss(pred, batch[f'voxel_label_{f}'], rays, n_valid, w_rc * (1 / f),
                                                                                terms=True)[0]
        # the distance-transform boundary loss of the voxel head (extension, config.py: LOSSES.VOXEL_BOUNDARY; absent = off: no
        # term, no launch), last for the same reason; like the Lovasz term it reads the visible labels when the mask is on - 255
        # cells are inert by its definition
        w_bd, bd_factors, bd_truncate = voxel_boundary(cfg)
        if w_bd > 0:
            for f in bd_factors:
                losses[f'voxel_boundary_{f}'] = ops.voxel_boundary_loss(output[f'voxel_{f}'], voxel_target(cfg, batch, f),
                                                                        voxel_boundary_cells(cfg, bd_truncate, f), w_bd * (1 / f), terms=True)[0]
        return losses

    def _seg_loss(self, tag, c, is_bev=False):
        """trainer.py:61-66,132-161: SegmentationLoss(use_top_k, top_k_ratio, use_weights, is_bev)."""
        from .losses import SegmentationLoss
        cache = self.__dict__.setdefault('_seg_losses', {})
        if tag not in cache:
            cache[tag] = SegmentationLoss(use_top_k=c.USE_TOP_K, top_k_ratio=c.TOP_K_RATIO, use_weights=c.USE_WEIGHTS, is_bev=is_bev)
        return cache[tag]

    def loss_reducing(self, loss):
        vals = list(loss.values())
        return ops.sum_scalars(vals)

    def training_step(self, batch, batch_idx=0, noise=None, use_prior=None):
        """trainer.py:392-402: switch the RSSM to active inference at batch STEPS, shared_step('train'), log the 21 terms,
        return their sum."""
        if batch_idx == self.cfg.STEPS and self.cfg.MODEL.TRANSITION.ENABLED:
            print('!' * 50)
            print('ACTIVE INFERENCE ACTIVATED')
            print('!' * 50)
            self.model.rssm.active_inference = True
        if self._optimizer is not None and self.model.seed_epoch != self._optimizer._step + 1:
            # dropout seeds = f(rank, optimizer step, micro-batch within the step): reproducible across a checkpoint resume
            self.model.seed_epoch = self._optimizer._step + 1
            self.model._step_seed = 0
        if self._reducer is not None:
            self._reducer.accumulating = self._is_accumulating()
            self._reducer.begin_step()
        losses, output, _, _ = self.shared_step(batch, mode='train', noise=noise, use_prior=use_prior)
        # kept detached: a loss tensor with its grad_fn would keep this step's autograd graph - and the AccumulateGrad nodes of
        # every parameter, created on the side streams - alive into the next step (memory, and PyTorch's stream-mismatch warning
        # as soon as a parameter is then used on another stream; Lightning's self.log detaches as well)
        self.last_losses = {k: v.detach() for k, v in losses.items()}
        self.logging_and_visualisation(batch, output, [], losses, None, batch_idx, prefix='train')
        return self.loss_reducing(losses)

    def logging_and_visualisation(self, batch, output, output_imagine, loss, loss_imagines, batch_idx, prefix='train'):
        """trainer.py:492-509: `self.log(f'{prefix}_{key}', value)` per loss term and `-global_step`, then - while `panel_writer`
        is set - `visualise` under the reference's criterion: in training on every step that is a multiple of
        LOG_VIDEO_INTERVAL, once per step (`vis_step`); otherwise on batch 0.  Under Lightning `self.log` is the
        LightningModule's; in a plain loop the values are handed to `self.log_fn(name, value)` if one is set, else kept (still
        device tensors: no host sync) in `self.logged`."""
        step = self._step_now()
        self.log('-global_step', torch.tensor(-float(step), dtype=torch.float32))
        for key, value in loss.items():
            self.log(f'{prefix}_{key}', value)
        if loss_imagines:
            for key, value in loss_imagines[0].items():
                self.log(f'{prefix}_{key}_imagine', value)
        if self.panel_writer is None:
            return
        if prefix == 'train':
            wanted = (step % self.cfg.LOG_VIDEO_INTERVAL == 0) and (step != self.vis_step)
            self.vis_step = step
        else:
            wanted = batch_idx == 0
        if wanted:
            self.visualise(batch, output, output_imagine, batch_idx, prefix=prefix)

    def _step_now(self):
        return getattr(self, 'global_step', 0) if pl is not None else self._global_step

    def visualise(self, batch, output, output_imagines, batch_idx, prefix='train', writer=None):
        """trainer.py:569-957: the picture grids of one batch (muvo_amd/visualise.py: which ones, and what is left out), rendered
        on the device from the tensors as they are, to `writer` (default `self.panel_writer`) as `{prefix}_outputs[_{batch_idx}]{suffix}`."""
        from muvo_amd.visualise import render_panels, write_panels
        writer = writer if writer is not None else self.panel_writer
        if writer is None:
            raise RuntimeError('visualise: no writer (set `panel_writer`, e.g. muvo_amd.visualise.PanelWriter(directory))')
        name = f'{prefix}_outputs'
        if prefix != 'train':
            name = name + f'_{batch_idx}'
        with torch.no_grad():
            panels = render_panels(self.cfg, batch, output, output_imagines)
        write_panels(writer, name, panels, self._step_now())
        if self.traj_panels and self.cfg.LIDAR_RE.ENABLED:
            from muvo_amd.odometry import traj_panel
            with torch.no_grad():
                writer.add_images(f'{name}_traj', traj_panel(self.cfg, batch, output, output_imagines, **self.traj_options), global_step=self._step_now())
        if self.flow_panels and self.cfg.EVAL.RGB_SUPERVISION:
            from muvo_amd.flow import flow_panel
            with torch.no_grad():
                writer.add_images(f'{name}_flow', flow_panel(batch, output, output_imagines), global_step=self._step_now())
        if getattr(self, 'voxel_panels', False) and self.cfg.VOXEL_SEG.ENABLED:
            from muvo_amd.voxel_view import voxel_panel
            with torch.no_grad():
                writer.add_images(f'{name}_voxel', voxel_panel(self.cfg, batch, output, output_imagines, **getattr(self, 'voxel_options', {})),
                                  global_step=self._step_now())
        if getattr(self, 'inst_panels', False) and self.cfg.SEMANTIC_SEG.ENABLED:
            from muvo_amd.bev_instances import inst_panel
            with torch.no_grad():
                writer.add_images(f'{name}_inst', inst_panel(self.cfg, batch, output, output_imagines, **getattr(self, 'inst_options', {})),
                                  global_step=self._step_now())
        if getattr(self, 'uncert_panels', False) and self.cfg.VOXEL_SEG.ENABLED:
            from muvo_amd.calibration import uncert_panel
            with torch.no_grad():
                writer.add_images(f'{name}_uncert', uncert_panel(self.cfg, batch, output, output_imagines), global_step=self._step_now())
        return panels

    if pl is None:
        def log(self, name, value, *args, **kwargs):
            if torch.is_tensor(value):
                value = value.detach()
            if self.log_fn is not None:
                self.log_fn(name, value)
            else:
                self.logged[name] = value

    # ------------------------------------------------------------------ data-parallel hooks (Lightning names)
    def on_before_zero_grad(self, optimizer=None):
        pass

    def on_after_backward(self):
        """Lightning calls this right after `loss.backward()`: send the gradient segments backward has not sent itself
        and make the optimizer's stream wait for the exchange.  A plain loop calls it between backward() and step()."""
        if self._reducer is not None:
            if self._reducer.accumulating:
                self._reducer.skip()          # gradients keep accumulating locally; exchanged after the last micro-batch
            else:
                self._reducer.finish()

    def _is_accumulating(self):
        """True for every micro-batch but the last of an ACCUMULATE_GRAD_BATCHES group: Lightning's loop knows
        (`_should_accumulate`); a plain loop sets `self.accumulate_now`."""
        if pl is not None and getattr(self, '_trainer', None) is not None:
            return bool(self._trainer.fit_loop.epoch_loop._should_accumulate())
        return bool(self.accumulate_now)

    def configure_ddp(self, *a, **k):   # pragma: no cover
        raise RuntimeError(_DDP_MSG)

    # ------------------------------------------------------------------ optimiser
    def configure_optimizers(self):
        cfg = self.cfg
        if cfg.OPTIMIZER.FROZEN.ENABLED:
            keep = tuple(cfg.OPTIMIZER.FROZEN.TRAIN_LIST)
            for name, param in self.model.named_parameters():
                if not name.startswith(keep):
                    param.requires_grad = False
        self.store = ParamStore(self.model)
        unused = [p for _, p in self.store.unused]
        optimizer = FusedAdamW(self.store, lr=cfg.OPTIMIZER.LR, weight_decay=cfg.OPTIMIZER.WEIGHT_DECAY,
                               extra_unused=unused)
        if cfg.SCHEDULER.NAME == 'none':
            sched = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda lr: 1)
        elif cfg.SCHEDULER.NAME == 'OneCycleLR':
            sched = torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=cfg.OPTIMIZER.LR, total_steps=cfg.STEPS,
                                                        pct_start=cfg.SCHEDULER.PCT_START)
        else:
            raise ValueError(cfg.SCHEDULER.NAME)
        self._optimizer = optimizer
        self._attach_reducer(optimizer)
        return [optimizer], [{'scheduler': sched, 'interval': 'step'}]

    def _attach_reducer(self, optimizer):
        """Data parallelism (reference: Lightning's implicit DDP, train.py:93-98).  When torch.distributed is initialised
        with more than one rank, the segmented reducer (muvo_amd/parallel.py) is attached here: backward hooks launch one
        RCCL all-reduce per finished segment on a side stream, `on_after_backward` waits for them, AdamW divides by the
        world size.  A DistributedDataParallel wrapper around this module would all-reduce a second time (and trip over
        the 12 never-used `encoder_layer.*` tensors): refuse it."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        from muvo_amd.parallel import SegmentedGradReducer
        self._reducer = SegmentedGradReducer(self.store)
        self.model.segment_done = self._reducer.segment_done
        self.model.dropout_rank = dist.get_rank()
        optimizer.grad_scale = self._reducer.grad_scale
        self.register_forward_pre_hook(_refuse_ddp)
