"""Predict over recorded runs with a trained checkpoint: the counterpart of the reference's two inference entry points,
`prediction.py` (`trainer.test` over the test loaders) and `sim_run.py` (`sim_forward` over test loader 2, dumping label,
reconstruction and imagination per batch).  One process, one GPU.

    python -m muvo_amd.predict --config-file muvo_amd/configs/test_base_1d.yml --dataset-root /data/carla \\
        --checkpoint epoch=0-step=50000.ckpt --out runs/eval --mode test
    python -m muvo_amd.predict --config-file muvo_amd/configs/test_base_1d.yml --dataset-root /data/carla \\
        --checkpoint epoch=0-step=50000.ckpt --out runs/sim --mode sim [--loader 2] [--limit-batches 100] [--shard-size 500]

`--mode test` runs `WorldModelTrainer.test_step` over the chosen test loaders (default: all three), then `on_test_epoch_end`,
prints every logged metric as a JSON line and writes `metrics.json` (with `--panels N` also the picture grids of the first N
batches of every loader, as PNG files below `OUT/panels`; muvo_amd/visualise.py): the logged names mapped to floats, plus `batches`, the
number of batches each loader delivered.  With the bird's-eye-view, lidar or camera segmentation head enabled the file also
holds that head's per-class and mean IoU (`{set}_{bev,lidar,camera}_iou_{class}`, `..._mean_iou`; the reference sends these to
the TensorBoard writer, here they arrive with the rest) and `{set}_{bev,lidar,camera}_confusion`: the C x C count matrix
[label][prediction] as nested integer lists.  The reference's class-name table has two entries, so only two of the lidar and
camera head's nine per-class scores carry a name; the matrix holds what the other seven are computed from.  The counts are
taken on the device (csrc/metrics.hip: argmax + confusion matrix in one kernel per head and batch) and read once at the end.
With that head on, `--bev-pq` also writes `bev_pq.json`, the panoptic quality of the instances decoded on the device from the
head's centre / offset outputs, and `--panels N --inst` the `_inst` panels (muvo_amd/bev_instances.py); `metrics.json` is the same
with and without them.  With the voxel head on, `--voxel-calibration` writes `voxel_calibration.json` - calibration, ensemble IoU and
uncertainty of that head over all imagined samples jointly - and `--panels N --uncert` the `_uncert` panels (muvo_amd/calibration.py);
`metrics.json` is again the same with and without them.

`--mode sim` follows the loop of sim_run.py:49-116 (module in train() mode, the transformer's dropout modules off, no_grad;
per batch `preprocess`, then `model.sim_forward(batch, is_dreaming=False)`) over one loader (default 2, sim_run.py:44) and
records, for batch element 0, the reference's eleven entries.  Every `--shard-size` batches, and at the end, a shard
`data_{i}.npz` is written, i = index of the last batch in it.

Shard layout (B batches in the shard, K = the steps of (0, 3, 9) the imagination has; arrays of a shard are stacked over B):

    rgb_label, rgb_re       (B, 3, h, w) uint8      frame 0 of the label / the rendered current state, muvo_image_u8
    rgb_im                  (B, K, 3, h, w) uint8   imagined steps
    throttle_brake, steering (B, 1) float32         recorded action of frame 0
    pcd_label, pcd_re       (B, 4, H, W) float32    range views, copied as they are
    pcd_im                  (B, K, 4, H, W) float32
    voxel_label_rows, voxel_re_rows, voxel_im_rows   (sum Q, 4) uint16   x, y, z, class of every voxel whose class is not 0
        (label: the uint8 grid itself; re / im: argmax of the logits), ascending in (x * Y + y) * Z + z - the order of
        torch.where, the layout of the recorder's voxel files
    voxel_label_offsets, voxel_re_offsets (B + 1,) int64, voxel_im_offsets (B * K + 1,) int64: entry j of the row list
        ((batch, step) in row-major order for `im`) owns rows [offsets[j], offsets[j + 1])
    imagine_steps (K,) int64, batch_index (B,) int64

Bytes are `trunc(x * 255)` saturated to [0, 255] with NaN -> 0: numpy's `(x * 255).astype(np.uint8)` of the reference
wherever that is defined.  Neither a logits tensor nor a float image crosses to the host: the voxel entries are compacted by
csrc/export.hip (class argmax + ordered stream compaction) and leave as rows, the images leave as bytes.  `read_shard` gives
the per-batch lists back."""
import json
import os
import sys

import numpy as np
import torch

from muvo_amd.config import get_cfg, get_parser

ENTRIES = ('rgb_label', 'throttle_brake', 'steering', 'pcd_label', 'voxel_label', 'rgb_re', 'pcd_re', 'voxel_re', 'rgb_im',
           'pcd_im', 'voxel_im')                       # sim_run.py:55-67
VOXEL_ENTRIES = ('voxel_label', 'voxel_re', 'voxel_im')
IMAGINE_STEPS = (0, 3, 9)                              # sim_run.py:81,92-93


SENSORS = ('camera', 'lidar')              # --drop-sensor; batch['sensor_drop'] codes 1, 2 (muvo_amd/models/mile.py)


def check_drop_sensor(cfg, drop_sensor):
    if drop_sensor is not None and drop_sensor not in SENSORS:
        raise ValueError(f'drop_sensor {drop_sensor!r}: camera or lidar')
    if drop_sensor is not None and not cfg.MODEL.TRANSFORMER.ENABLED:
        raise ValueError('--drop-sensor hides tokens in the fusion transformer: it needs MODEL.TRANSFORMER.ENABLED')


def set_sensor_drop(cfg, batch, drop_sensor):
    """batch['sensor_drop'] = the code of `drop_sensor` ('camera' | 'lidar') for every sequence of the batch; None: nothing"""
    check_drop_sensor(cfg, drop_sensor)
    if drop_sensor is None:
        return batch
    batch['sensor_drop'] = torch.full((batch['image'].shape[0],), SENSORS.index(drop_sensor) + 1, dtype=torch.int8)
    return batch


def refuse_multi_process(environ=None):
    environ = os.environ if environ is None else environ
    world = int(environ.get('WORLD_SIZE', '1') or 1)
    if world > 1:
        raise RuntimeError(f'muvo_amd.predict runs in one process on one GPU (WORLD_SIZE={world}): start it without a launcher; '
                           'multi-process evaluation is not built')


def build_parser():
    parser = get_parser()
    parser.description = 'World model prediction over recorded runs'
    parser.add_argument('--dataset-root', default='', help='directory of recorded runs (overrides DATASET.DATAROOT)')
    parser.add_argument('--checkpoint', default='', help='Lightning-format checkpoint (goes to PRETRAINED.PATH)')
    parser.add_argument('--out', required=True, metavar='DIR', help='directory for metrics.json / data_{i}.npz')
    parser.add_argument('--mode', choices=('test', 'sim'), required=True)
    parser.add_argument('--loader', type=int, choices=(0, 1, 2), default=None,
                        help='test loader (default: 2 for sim, all three for test)')
    parser.add_argument('--limit-batches', type=int, default=None, metavar='N', help='at most N batches per loader')
    parser.add_argument('--shard-size', type=int, default=500, metavar='N', help='batches per data_{i}.npz (sim)')
    parser.add_argument('--seed', type=int, default=1234)
    parser.add_argument('--drop-sensor', choices=SENSORS, default=None,
                        help="every sample runs without that sensor: its tokens are blanked and hidden from the fusion transformer's "
                             "attention (batch['sensor_drop']); metrics.json gains a \"drop_sensor\" entry")
    parser.add_argument('--panels', type=int, default=0, metavar='N',
                        help='test: write the picture grids of the first N batches per loader below OUT/panels (default: none)')
    parser.add_argument('--traj', action='store_true', help='with --panels: also the ego-trajectory panel `_traj` (ICP between lidar frames)')
    parser.add_argument('--flow', action='store_true', help='with --panels: also the optical-flow panel `_flow` (dense Farneback flow between camera frames)')
    parser.add_argument('--optical-flow', action='store_true',
                        help='test: endpoint error between the flow of the recorded and of the predicted camera frames -> OUT/optical_flow.json')
    parser.add_argument('--voxel', action='store_true', help='with --panels: also the 3-D voxel panel `_voxel` (the grids ray-cast on the device)')
    parser.add_argument('--voxel-size', type=int, default=256, metavar='R', help='--voxel: pixels a side of one tile (default 256)')
    parser.add_argument('--ray-iou', action='store_true',
                        help='test: ray-based IoU of the voxel head (first hits of lidar-like rays through label and prediction) -> OUT/ray_iou.json')
    parser.add_argument('--ray-stride', type=int, default=4, metavar='K', help='--ray-iou: every K-th azimuth of the range view is a ray (default 4)')
    parser.add_argument('--voxel-cd', action='store_true',
                        help='test: Chamfer distance and F-scores at 1 / 2 / 4 m between the occupied cells of voxel label and prediction -> OUT/voxel_cd.json')
    parser.add_argument('--bev-pq', action='store_true',
                        help='test: panoptic quality of the instances decoded from the BEV centre / offset heads -> OUT/bev_pq.json')
    parser.add_argument('--inst', action='store_true', help='with --panels: also the BEV instance panel `_inst` (label ids and decoded ids)')
    parser.add_argument('--inst-threshold', type=float, default=0.1, metavar='T', help='--bev-pq / --inst: a centre is a peak above T (default 0.1)')
    parser.add_argument('--inst-max-centres', type=int, default=100, metavar='K', help='--bev-pq / --inst: at most K centres per frame (default 100; 1..254)')
    parser.add_argument('--voxel-calibration', action='store_true',
                        help='test: calibration (ECE, reliability, Brier, NLL), ensemble IoU and uncertainty of the voxel head over all imagined samples -> OUT/voxel_calibration.json')
    parser.add_argument('--calibration-bins', type=int, default=15, metavar='B', help='--voxel-calibration: equal-width confidence bins (default 15; 1..32)')
    parser.add_argument('--uncert', action='store_true',
                        help='with --panels: also the uncertainty panel `_uncert` (top views of the predictive entropy and the mutual information)')
    parser.add_argument('--ego-motion', action='store_true',
                        help='test: drift of the ego path implied by the predicted lidar from the one implied by the recorded lidar -> OUT/ego_motion.json')
    parser.add_argument('--ego-threshold', type=float, default=5.0, metavar='M', help='ICP inlier distance in metres of --ego-motion and --traj (default 5, the reference)')
    parser.add_argument('--ego-stride', type=int, default=1, metavar='K', help='every K-th source point is an ICP query (default 1: exact)')
    parser.add_argument('--ego-search', choices=('brute', 'grid'), default='brute',
                        help='neighbour search of the ICP of --ego-motion and --traj (default brute; grid: a cell grid of the target points, the same result bit for bit)')
    parser.add_argument('--ego-max-iteration', type=int, default=2000, metavar='N', help='ICP iteration cap (default 2000, the reference)')
    return parser


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.limit_batches is not None and args.limit_batches < 1:
        raise SystemExit('--limit-batches must be positive')
    if args.shard_size < 1:
        raise SystemExit('--shard-size must be positive')
    if args.panels < 0 or (args.panels and args.mode != 'test'):
        raise SystemExit('--panels takes a non-negative count and goes with --mode test')
    if (args.ego_motion or args.traj) and args.mode != 'test':
        raise SystemExit('--ego-motion and --traj go with --mode test')
    if args.traj and not args.panels:
        raise SystemExit('--traj goes with --panels N')
    if (args.flow or args.optical_flow) and args.mode != 'test':
        raise SystemExit('--flow and --optical-flow go with --mode test')
    if args.flow and not args.panels:
        raise SystemExit('--flow goes with --panels N')
    if (args.voxel or args.ray_iou) and args.mode != 'test':
        raise SystemExit('--voxel and --ray-iou go with --mode test')
    if args.voxel_cd and args.mode != 'test':
        raise SystemExit('--voxel-cd goes with --mode test')
    if args.voxel and not args.panels:
        raise SystemExit('--voxel goes with --panels N')
    if (args.bev_pq or args.inst) and args.mode != 'test':
        raise SystemExit('--bev-pq and --inst go with --mode test')
    if args.inst and not args.panels:
        raise SystemExit('--inst goes with --panels N')
    if not 1 <= args.inst_max_centres <= 254 or args.inst_threshold != args.inst_threshold:
        raise SystemExit('--inst-max-centres lies in 1..254 and --inst-threshold is a number')
    if (args.voxel_calibration or args.uncert) and args.mode != 'test':
        raise SystemExit('--voxel-calibration and --uncert go with --mode test')
    if args.uncert and not args.panels:
        raise SystemExit('--uncert goes with --panels N')
    if not 1 <= args.calibration_bins <= 32:
        raise SystemExit('--calibration-bins lies in 1..32')
    if args.voxel_size < 1 or args.ray_stride < 1:
        raise SystemExit('--voxel-size and --ray-stride must be positive')
    if args.ego_threshold <= 0 or args.ego_stride < 1 or args.ego_max_iteration < 0:
        raise SystemExit('--ego-threshold must be positive, --ego-stride at least 1, --ego-max-iteration non-negative')
    return args


def chosen_loaders(mode, loader=None):
    return [int(loader)] if loader is not None else ([2] if mode == 'sim' else [0, 1, 2])


def expected_metric_names(cfg, counts):
    """The names `on_test_epoch_end` logs when loader idx delivered counts[idx] batches (an empty loader logs nothing)."""
    from muvo_amd.trainer import metric_names
    names = []
    for kind, has in (('test', True), ('test_imagine', cfg.PREDICTION.N_SAMPLES > 0)):
        for idx in sorted(counts):
            if counts[idx] and has:
                names += metric_names(cfg, f'{kind}{idx}')
    return names


# ---- shards -----------------------------------------------------------------------------------------------------------------------
def write_shard(path, records, batch_index, imagine_steps):
    """records: one dict per batch with the ENTRIES; fixed-shape entries are numpy arrays, `voxel_label` / `voxel_re` a (Q, 4)
    uint16 array, `voxel_im` a list of K such arrays."""
    out = {'imagine_steps': np.asarray(imagine_steps, dtype=np.int64), 'batch_index': np.asarray(batch_index, dtype=np.int64)}
    for name in ENTRIES:
        if name in VOXEL_ENTRIES:
            lists = [r[name] if name == 'voxel_im' else [r[name]] for r in records]
            flat = [np.asarray(a, dtype=np.uint16).reshape(-1, 4) for per_batch in lists for a in per_batch]
            out[f'{name}_rows'] = np.concatenate(flat) if flat else np.zeros((0, 4), np.uint16)
            out[f'{name}_offsets'] = np.concatenate([[0], np.cumsum([len(a) for a in flat])]).astype(np.int64)
        else:
            out[name] = np.stack([np.asarray(r[name]) for r in records])
    with open(path, 'wb') as fh:
        np.savez(fh, **out)
    return path


def read_shard(path):
    """The per-batch lists of a shard: {entry: list over the batches}; a voxel entry is a (Q, 4) uint16 array per batch
    (`voxel_im`: a list of K arrays per batch).  Plus `imagine_steps` and `batch_index`."""
    with np.load(path) as z:
        data = {k: z[k] for k in z.files}
    n, k = len(data['batch_index']), len(data['imagine_steps'])
    out = {'imagine_steps': data['imagine_steps'], 'batch_index': data['batch_index']}
    for name in ENTRIES:
        if name in VOXEL_ENTRIES:
            rows, off = data[f'{name}_rows'], data[f'{name}_offsets']
            parts = [rows[off[j]:off[j + 1]] for j in range(len(off) - 1)]
            out[name] = [parts[i * k:(i + 1) * k] for i in range(n)] if name == 'voxel_im' else parts
            assert len(out[name]) == n, (name, len(parts), n, k)
        else:
            out[name] = list(data[name])
    return out


def _split_rows(rows, counts):
    host = rows.cpu().numpy()
    edges = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [host[edges[j]:edges[j + 1]] for j in range(len(counts))]


def sim_record(batch, output, output_imagine):
    """The eleven entries of sim_run.py:75-94 for batch element 0 from device tensors; returns (record, imagined steps)."""
    from muvo_amd import ops
    n_im = output_imagine['voxel_1'].shape[1] if output_imagine else 0
    steps = [k for k in IMAGINE_STEPS if k < n_im]
    idx = torch.as_tensor(steps, dtype=torch.long, device=output['voxel_1'].device)
    rec = {'throttle_brake': batch['throttle_brake'][0][0].float().cpu().numpy(),
           'steering': batch['steering'][0][0].float().cpu().numpy(),
           'rgb_label': ops.image_u8(batch['rgb_label_1'][0][0].float()).cpu().numpy(),
           'rgb_re': ops.image_u8(output['rgb_1'][0][0].detach().float()).cpu().numpy(),
           'pcd_label': batch['range_view_label_1'][0][0].float().cpu().numpy(),
           'pcd_re': output['lidar_reconstruction_1'][0][0].detach().float().cpu().numpy()}
    label = batch['voxel_label_1'][0][0]
    label = label.reshape(1, *label.shape[-3:]).to(torch.uint8)
    rec['voxel_label'] = _split_rows(*ops.voxel_rows(label))[0]
    rec['voxel_re'] = _split_rows(*ops.voxel_rows(output['voxel_1'][0][0:1].detach().float()))[0]
    if steps:
        rec['rgb_im'] = ops.image_u8(output_imagine['rgb_1'][0].detach().float().index_select(0, idx)).cpu().numpy()
        rec['pcd_im'] = output_imagine['lidar_reconstruction_1'][0].detach().float().index_select(0, idx).cpu().numpy()
        rec['voxel_im'] = _split_rows(*ops.voxel_rows(output_imagine['voxel_1'][0].detach().float().index_select(0, idx)))
    else:
        rec['rgb_im'] = np.zeros((0, *rec['rgb_re'].shape), np.uint8)
        rec['pcd_im'] = np.zeros((0, *rec['pcd_re'].shape), np.float32)
        rec['voxel_im'] = []
    return rec, steps


# ---- the two modes ----------------------------------------------------------------------------------------------------------------
def _check_heads(cfg, mode):
    on = {'EVAL.RGB_SUPERVISION': cfg.EVAL.RGB_SUPERVISION, 'LIDAR_RE.ENABLED': cfg.LIDAR_RE.ENABLED,
          'VOXEL_SEG.ENABLED': cfg.VOXEL_SEG.ENABLED}
    off = [k for k, v in on.items() if not v]
    if mode == 'sim' and off:
        raise RuntimeError(f'--mode sim records the RGB, lidar and voxel outputs (sim_run.py:84-94): {off} must be on')


def seed_batch(module, seed, loader_idx, i):
    """Every batch starts from seeds of its own - torch (RSSM noise), numpy (the Chamfer subset, trainer.py:453) and the model's
    dropout counters - so a run does not depend on what the module did before, and a second run repeats the first."""
    s = seed + 104729 * (i + 1) + 7919 * loader_idx
    torch.manual_seed(s)
    np.random.seed(s % (2 ** 32))
    module.model.seed_epoch = 0
    module.model._step_seed = ((loader_idx << 20) + i) << 8


def run(cfg, device, out_dir, mode, loaders=None, limit_batches=None, shard_size=500, seed=1234, hook=None, dataset_root=None,
        data=None, module=None, log=print, panels=0, traj=False, ego_motion=None, icp_options=None, flow=False, optical_flow=False,
        voxel=False, voxel_size=256, ray_iou=None, voxel_cd=None, bev_pq=None, inst=False, voxel_calibration=None, uncert=False,
        drop_sensor=None):
    """Runs one mode and returns what it wrote: {'files': [...], 'batches': {loader: n}, 'metrics': {...}, 'confusion': {...} (test)}.
    hook(i, batch, output, output_imagine): called per batch with the device tensors (test mode: output_imagine is the list
    of imagined samples).  data: a set-up DataModule to take the test loaders from (default: one over dataset_root /
    cfg.DATASET.DATAROOT); module: a WorldModelTrainer to use instead of building one from cfg.  panels (test): the picture grids
    of the first `panels` batches of every loader go to PNG files below out_dir/panels (muvo_amd/visualise.py), with traj also
    `_traj`.  ego_motion (test): dict(threshold, stride, max_iteration, search) - muvo_amd.odometry.EgoMotionMetric runs behind `hook` on every
    batch and writes out_dir/ego_motion.json; metrics.json does not change.  icp_options: dict(threshold, source_stride,
    max_iteration) of the ICP behind the `_traj` panel (default: 5 m, 1, 2000).  flow (test, with panels): also the `_flow` panel;
    optical_flow (test): muvo_amd.flow.FlowMetric runs on every batch and writes out_dir/optical_flow.json; metrics.json does
    not change.  voxel (test, with panels): also the `_voxel` panel with tiles of voxel_size pixels; ray_iou (test): dict(stride) -
    muvo_amd.voxel_view.RayIoUMetric runs on every batch and writes out_dir/ray_iou.json; metrics.json does not change.  voxel_cd
    (test): a dict (empty: no options) - muvo_amd.voxel_view.VoxelDistanceMetric runs on every batch and writes
    out_dir/voxel_cd.json; metrics.json does not change.  bev_pq (test): a dict of decode options (threshold, radius, max_centres,
    thing_classes; empty: the defaults) - muvo_amd.bev_instances.PanopticQualityMetric runs on every batch and writes
    out_dir/bev_pq.json; metrics.json does not change.  inst (test, with panels): also the `_inst` panel - True: decoded with the
    options of bev_pq (the defaults without it); a dict: with decode options of its own.  voxel_calibration (test): a dict of options
    (bins; empty: 15) - muvo_amd.calibration.VoxelCalibrationMetric runs on every batch and writes out_dir/voxel_calibration.json;
    metrics.json does not change.  uncert (test, with panels): also the `_uncert` panel.  drop_sensor (test and sim): 'camera' or
    'lidar' - every batch gets `batch['sensor_drop']` for all its sequences (muvo_amd/models/mile.py: the sensor's tokens are
    blanked and are no attention keys); the file names stay, metrics.json gains the entry "drop_sensor"."""
    refuse_multi_process()
    check_drop_sensor(cfg, drop_sensor)                                          # refused here, before anything is built
    if mode not in ('test', 'sim'):
        raise ValueError(f'mode {mode!r}: test or sim')
    _check_heads(cfg, mode)
    device = torch.device(device)
    os.makedirs(out_dir, exist_ok=True)
    torch.manual_seed(seed)
    if module is None:
        from muvo_amd.trainer import WorldModelTrainer
        module = WorldModelTrainer(cfg.convert_to_dict(), device=device)
    if data is None:
        from muvo_amd.data.dataset import DataModule
        data = DataModule(cfg, dataset_root or cfg.DATASET.DATAROOT, device=device, seed=seed)
        data.setup()
    test_loaders = data.test_dataloader()
    which = chosen_loaders(mode, None) if loaders is None else [int(v) for v in loaders]
    if mode == 'sim' and len(which) != 1:
        raise ValueError('mode sim runs over one loader')
    chosen = {idx: test_loaders[idx] for idx in which}
    if mode == 'sim':
        if panels or traj or ego_motion is not None or flow or optical_flow or voxel or ray_iou is not None:
            raise ValueError('panels, the ego-motion metric, the optical-flow metric and the ray IoU belong to mode test')
        if voxel_cd is not None:
            raise ValueError('the voxel Chamfer distance belongs to mode test')
        if bev_pq is not None or isinstance(inst, dict) or inst:
            raise ValueError('the BEV panoptic quality and the `_inst` panel belong to mode test')
        if voxel_calibration is not None or uncert:
            raise ValueError('the voxel calibration and the `_uncert` panel belong to mode test')
        return _run_sim(cfg, module, chosen, out_dir, limit_batches, shard_size, seed, hook, log, drop_sensor)
    return _run_test(cfg, module, chosen, out_dir, limit_batches, shard_size, seed, hook, log, panels, traj, ego_motion, icp_options, flow, optical_flow,
                     voxel, voxel_size, ray_iou, voxel_cd, bev_pq, inst, voxel_calibration, uncert, drop_sensor)


def _batches(loader, limit):
    for i, batch in enumerate(loader):
        if limit is not None and i >= limit:
            return
        yield i, batch


def _run_test(cfg, module, loaders, out_dir, limit_batches, shard_size, seed, hook, log, panels=0, traj=False, ego_motion=None, icp_options=None,
              flow=False, optical_flow=False, voxel=False, voxel_size=256, ray_iou=None, voxel_cd=None, bev_pq=None, inst=False, voxel_calibration=None, uncert=False,
              drop_sensor=None):
    counts = {}
    writer, was_writer, was_traj, was_opt = None, module.panel_writer, module.traj_panels, module.traj_options
    ego, flow_metric, was_flow = None, None, module.flow_panels
    ray_metric, was_voxel, was_vopt = None, module.voxel_panels, module.voxel_options
    if (voxel or ray_iou is not None) and not cfg.VOXEL_SEG.ENABLED:
        raise ValueError('the ray IoU and the `_voxel` panel need the voxel head (VOXEL_SEG.ENABLED)')
    if voxel_cd is not None and not cfg.VOXEL_SEG.ENABLED:
        raise ValueError('the voxel Chamfer distance needs the voxel head (VOXEL_SEG.ENABLED)')
    if (bev_pq is not None or isinstance(inst, dict) or inst) and not cfg.SEMANTIC_SEG.ENABLED:
        raise ValueError('the BEV panoptic quality and the `_inst` panel need the bird\'s-eye-view head (SEMANTIC_SEG.ENABLED)')
    if (voxel_calibration is not None or uncert) and not cfg.VOXEL_SEG.ENABLED:
        raise ValueError('the voxel calibration and the `_uncert` panel need the voxel head (VOXEL_SEG.ENABLED)')
    cal_metric, was_uncert = None, getattr(module, 'uncert_panels', False)
    if voxel_calibration is not None:
        from muvo_amd.calibration import VoxelCalibrationMetric
        cal_metric = VoxelCalibrationMetric(cfg, **voxel_calibration)
    inst_on = isinstance(inst, dict) or bool(inst)
    pq_metric, was_inst, was_iopt = None, getattr(module, 'inst_panels', False), getattr(module, 'inst_options', {})
    if bev_pq is not None:
        from muvo_amd.bev_instances import PanopticQualityMetric
        pq_metric = PanopticQualityMetric(cfg, **bev_pq)
    if inst_on:                              # a dict: the panel's own decode options; True: those of the metric, else the defaults
        module.inst_options = dict(inst) if isinstance(inst, dict) else dict(bev_pq or {})
    cd_metric = None
    if voxel_cd is not None:
        from muvo_amd.voxel_view import VoxelDistanceMetric
        cd_metric = VoxelDistanceMetric(cfg, **voxel_cd)
    if ray_iou is not None:
        from muvo_amd.voxel_view import RayIoUMetric
        ray_metric = RayIoUMetric(cfg, **ray_iou)
    if voxel:
        module.voxel_options = dict(size=int(voxel_size))
    if (flow or optical_flow) and not cfg.EVAL.RGB_SUPERVISION:
        raise ValueError('the optical-flow metric and the `_flow` panel need the camera head (EVAL.RGB_SUPERVISION)')
    if optical_flow:
        from muvo_amd.flow import FlowMetric
        flow_metric = FlowMetric(cfg)
    if (ego_motion is not None or traj) and not cfg.LIDAR_RE.ENABLED:
        raise ValueError('the ego-motion metric and the `_traj` panel need the lidar reconstruction head (LIDAR_RE.ENABLED)')
    if ego_motion is not None:
        from muvo_amd.odometry import EgoMotionMetric
        ego = EgoMotionMetric(cfg, **ego_motion)
    if traj:                                 # the same ICP knobs for the panel
        module.traj_options = dict(icp_options or {})
    if panels:
        from muvo_amd.visualise import PanelWriter
        writer = PanelWriter(os.path.join(out_dir, 'panels'))
    try:
        for idx, loader in loaders.items():
            counts[idx] = 0
            if ego is not None:
                ego.start_loader(idx)
            if flow_metric is not None:
                flow_metric.start_loader(idx)
            if ray_metric is not None:
                ray_metric.start_loader(idx)
            if cd_metric is not None:
                cd_metric.start_loader(idx)
            if pq_metric is not None:
                pq_metric.start_loader(idx)
            if cal_metric is not None:
                cal_metric.start_loader(idx)
            for i, batch in _batches(loader, limit_batches):
                seed_batch(module, seed, idx, i)
                module.panel_writer = writer if i < panels else None
                module.traj_panels = bool(traj)
                module.flow_panels = bool(flow)
                module.voxel_panels = bool(voxel)
                if inst_on:
                    module.inst_panels = True
                if uncert:
                    module.uncert_panels = True
                output, output_imagines = module.test_step(set_sensor_drop(cfg, batch, drop_sensor), i, idx)
                if hook is not None:
                    hook(i, batch, output, output_imagines)
                if ego is not None:
                    ego.update(i, batch, output, output_imagines)
                if flow_metric is not None:
                    flow_metric.update(i, batch, output, output_imagines)
                if ray_metric is not None:
                    ray_metric.update(i, batch, output, output_imagines)
                if cd_metric is not None:
                    cd_metric.update(i, batch, output, output_imagines)
                if pq_metric is not None:
                    pq_metric.update(i, batch, output, output_imagines)
                if cal_metric is not None:
                    cal_metric.update(i, batch, output, output_imagines)
                counts[idx] += 1
    finally:
        module.panel_writer, module.traj_panels, module.traj_options, module.flow_panels = was_writer, was_traj, was_opt, was_flow
        module.voxel_panels, module.voxel_options = was_voxel, was_vopt
        if inst_on:
            module.inst_panels, module.inst_options = was_inst, was_iopt
        if uncert:
            module.uncert_panels = was_uncert
    logged, confusion = {}, {}
    was_fn, module.log_fn = module.log_fn, lambda name, value: logged.__setitem__(name, float(value))
    was_cm, module.on_confusion = module.on_confusion, lambda name, matrix: confusion.__setitem__(name, matrix.tolist())
    try:
        module.on_test_epoch_end()
    finally:
        module.log_fn, module.on_confusion = was_fn, was_cm
    result = {**logged, **confusion}
    result['batches'] = {str(idx): n for idx, n in counts.items()}
    if drop_sensor is not None:
        result['drop_sensor'] = drop_sensor
    for name, value in result.items():
        if name not in ('batches', 'drop_sensor'):
            log(json.dumps({name: value}))
    log(json.dumps({'batches': result['batches']}))
    path = os.path.join(out_dir, 'metrics.json')
    with open(path, 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write('\n')
    files = [path] + (writer.files if writer is not None else [])
    out = {'files': files, 'batches': counts, 'metrics': logged, 'confusion': confusion}
    if ego is not None:
        files.append(ego.write(out_dir))
        out['ego_motion'] = ego.result()
        log(json.dumps({'ego_motion': out['ego_motion']}))
    if flow_metric is not None:
        files.append(flow_metric.write(out_dir))
        out['optical_flow'] = flow_metric.result()
        log(json.dumps({'optical_flow': out['optical_flow']}))
    if ray_metric is not None:
        files.append(ray_metric.write(out_dir))
        out['ray_iou'] = ray_metric.result()
        log(json.dumps({'ray_iou': out['ray_iou']}))
    if cd_metric is not None:
        files.append(cd_metric.write(out_dir))
        out['voxel_cd'] = cd_metric.result()
        log('voxel_cd ' + json.dumps(out['voxel_cd'], sort_keys=True))
    if pq_metric is not None:
        files.append(pq_metric.write(out_dir))
        out['bev_pq'] = pq_metric.result()
        log('bev_pq ' + json.dumps(out['bev_pq'], sort_keys=True))
    if cal_metric is not None:
        files.append(cal_metric.write(out_dir))
        out['voxel_calibration'] = cal_metric.result()
        log('voxel_calibration ' + json.dumps(out['voxel_calibration'], sort_keys=True))
    return out


def _run_sim(cfg, module, loaders, out_dir, limit_batches, shard_size, seed, hook, log, drop_sensor=None):
    (idx, loader), = loaders.items()
    module.train()
    m = module.model
    m.last_h = m.last_sample = m.last_action = None       # the latent memory of sim_forward starts empty, like a fresh process
    m.count = 0
    layers = list(module.model.transformer_encoder.layers)
    saved = [getattr(layer, 'module_dropout_off', False) for layer in layers]
    for layer in layers:
        layer.module_dropout_off = True
    files, records, index, steps_of_shard, n = [], [], [], None, 0

    def flush():
        nonlocal records, index, steps_of_shard
        if records:
            files.append(write_shard(os.path.join(out_dir, f'data_{index[-1]}.npz'), records, index, steps_of_shard))
            log(json.dumps({'shard': files[-1], 'batches': len(records)}))
        records, index, steps_of_shard = [], [], None
    try:
        with torch.no_grad():
            for i, batch in _batches(loader, limit_batches):
                seed_batch(module, seed, idx, i)
                batch = set_sensor_drop(cfg, module.preprocess(batch), drop_sensor)
                output, output_imagine = module.model.sim_forward(batch, is_dreaming=False)
                if hook is not None:
                    hook(i, batch, output, output_imagine)
                rec, steps = sim_record(batch, output, output_imagine)
                if steps_of_shard is not None and steps != steps_of_shard:
                    flush()                                   # arrays of a shard are stacked: one set of steps per shard
                steps_of_shard = steps
                records.append(rec)
                index.append(i)
                n += 1
                if len(records) >= shard_size:
                    flush()
        flush()
    finally:
        for layer, v in zip(layers, saved):
            layer.module_dropout_off = v
    return {'files': files, 'batches': {idx: n}, **({'drop_sensor': drop_sensor} if drop_sensor is not None else {})}


def main(argv=None):
    args = parse_args(argv)
    refuse_multi_process()
    cfg = get_cfg(args)
    if args.checkpoint:
        cfg.defrost()
        cfg.PRETRAINED.PATH = args.checkpoint
        cfg.freeze()
    torch.cuda.set_device(0)
    device = torch.device('cuda', 0)
    run(cfg, device, args.out, args.mode, loaders=chosen_loaders(args.mode, args.loader), limit_batches=args.limit_batches,
        shard_size=args.shard_size, seed=args.seed, dataset_root=args.dataset_root or None, panels=args.panels, traj=args.traj,
        ego_motion=dict(threshold=args.ego_threshold, stride=args.ego_stride, max_iteration=args.ego_max_iteration, search=args.ego_search) if args.ego_motion else None,
        icp_options=dict(threshold=args.ego_threshold, source_stride=args.ego_stride, max_iteration=args.ego_max_iteration, search=args.ego_search),
        flow=args.flow, optical_flow=args.optical_flow, voxel=args.voxel, voxel_size=args.voxel_size,
        ray_iou=dict(stride=args.ray_stride) if args.ray_iou else None, voxel_cd={} if args.voxel_cd else None,
        bev_pq=dict(threshold=args.inst_threshold, max_centres=args.inst_max_centres) if args.bev_pq else None,
        inst=dict(threshold=args.inst_threshold, max_centres=args.inst_max_centres) if args.inst else False,
        voxel_calibration=dict(bins=args.calibration_bins) if args.voxel_calibration else None, uncert=args.uncert,
        drop_sensor=args.drop_sensor)


if __name__ == '__main__':
    sys.exit(main())
