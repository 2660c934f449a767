"""Thin counterpart of the reference's `train.py` (train.py:51-115) for the MI355X step: same command line
(`muvo/config.py:326-369`: `--config-file`, trailing `opts`), the plain loop that Lightning's automatic optimisation runs on a
LightningModule — training_step -> zero_grad -> backward -> (gradient exchange) -> optimizer.step -> scheduler.step with
`OPTIMIZER.ACCUMULATE_GRAD_BATCHES` micro-batches per step — the per-step loss log (trainer.py:492-499) and the checkpoint
callback: every `VAL_CHECK_INTERVAL` steps a Lightning-format checkpoint is written INTO THE CURRENT WORKING DIRECTORY under
Lightning's file name (`MyModelCheckpoint`, train.py:31-48: `filename = filepath.split('/')[-1]`).

With a data root (`DATASET.DATAROOT` or `--dataset-root`) the batches come from recorded CARLA runs through
`muvo_amd.data.dataset.DataModule` (host threads read and decode the files ahead of the step, the GPU prepares the frames of a batch in a
handful of launches); without one they are synthetic with the reference's batch schema (`muvo_amd/data/synthetic.py`).
One process per GPU; under `torch.distributed.run` the ranks form an RCCL group and
`WorldModelTrainer` exchanges gradients itself (muvo_amd/parallel.py) — no DistributedDataParallel wrapper.

    python -m muvo_amd.train --config-file muvo_amd/configs/test_base_1d.yml STEPS 100 BATCHSIZE 2 [--resume epoch=0-step=50.ckpt]
    python -m muvo_amd.train --config-file muvo_amd/configs/test_base_1d.yml --dataset-root /data/carla STEPS 100 BATCHSIZE 2
"""
import json
import os
import sys
import time

import torch

from muvo_amd.config import get_cfg, get_parser
from muvo_amd.data.synthetic import make_batch
from muvo_amd.trainer import WorldModelTrainer


def checkpoint_dict(module, optimizer, scheduler, global_step):
    """What Lightning's `dump_checkpoint` writes for this module (the keys the reference reads back: `state_dict` with the
    `model.` prefix, trainer.py:202-211; optimizer / scheduler states for resuming)."""
    return {'epoch': 0, 'global_step': global_step, 'pytorch-lightning_version': 'muvo_amd-plain-loop',
            'state_dict': module.state_dict(), 'optimizer_states': [optimizer.state_dict()],
            'lr_schedulers': [scheduler.state_dict()], 'hyper_parameters': {'hparams': module.cfg.convert_to_dict()},
            'world_size': int(os.environ.get('WORLD_SIZE', '1'))}


def save_checkpoint(module, optimizer, scheduler, global_step, save_dir):
    filepath = os.path.join(save_dir, f'epoch=0-step={global_step}.ckpt')
    filename = filepath.split('/')[-1]            # train.py:33: the file lands in the current working directory
    torch.save(checkpoint_dict(module, optimizer, scheduler, global_step), filename)
    return filename


def load_checkpoint(module, optimizer, scheduler, path):
    ck = torch.load(path, map_location='cpu', weights_only=False)
    # like load_pretrained_weights (trainer.py:202-211): the `model.` entries, strict; whatever else a Lightning checkpoint of
    # the reference carries in `state_dict` (loss-module buffers) is not needed
    module.model.load_state_dict({k[6:]: v for k, v in ck['state_dict'].items() if k[:6] == 'model.'}, strict=True)
    optimizer.load_state_dict(ck['optimizer_states'][0])
    scheduler.load_state_dict(ck['lr_schedulers'][0])
    return int(ck['global_step'])


def fit(cfg, device, steps=None, resume=None, log=None, seed=1234, batch_fn=None, setup=None, dataset_root=None, input_stream=False,
        panel_dir=None, traj=False, traj_options=None, validate=False, limit_val_batches=3, sanity_val_steps=2, val_batch_fn=None, metrics_log=None,
        flow=False, voxel=False, voxel_size=256, inst=False, uncert=False):
    """The training loop; returns (module, list of per-step loss dicts as floats).  batch_fn(micro_index) / setup(module):
    hooks for tests (own batches, e.g. switching dropout off).  dataset_root (default: cfg.DATASET.DATAROOT): batches from the
    recordings below it instead of synthetic ones; input_stream=True prepares them on a side stream instead of the main one.
    panel_dir: rank 0 writes the picture grids (muvo_amd/visualise.py) of every LOG_VIDEO_INTERVAL-th step there as PNG files;
    traj: also the `_traj` panel (muvo_amd/odometry.py: the ego path from on-device ICP between consecutive lidar frames);
    traj_options: dict(threshold, source_stride, max_iteration, search) of that ICP.  An untrained head is its worst case (tens of
    iterations per pair at every 64 x 1024 frame): the command line defaults to every 4th point and 200 iterations.
    flow: also the `_flow` panel (muvo_amd/flow.py: dense optical flow between consecutive camera frames, on the device).
    voxel: also the `_voxel` panel (muvo_amd/voxel_view.py: the voxel grids ray-cast in 3-D on the device), tiles of voxel_size pixels.
    inst: also the `_inst` panel (muvo_amd/bev_instances.py: the instances decoded from the BEV centre / offset heads, on the device).
    uncert: also the `_uncert` panel (muvo_amd/calibration.py: top views of the voxel head's predictive entropy and mutual information);
    it needs the voxel head (VOXEL_SEG.ENABLED), a ValueError otherwise.

    validate=True (train.py:104-110 under Lightning): before the first step a sanity pass of `sanity_val_steps` batches per
    validation loader whose results are dropped (not in a resumed run); after every optimizer step that is a multiple of
    VAL_CHECK_INTERVAL - and after that step's checkpoint is written, Lightning's order - one pass of
    `muvo_amd.validate.run_validation` over the first `limit_val_batches` batches of every loader.  The loaders: `val_batch_fn(idx)`
    -> iterable, asked again at every pass (idx 0, 1, 2; None or nothing to iterate: no such loader); else the three of
    `DataModule.val_dataloader()` below dataset_root; else one loader of synthetic batches whose seeds no training batch has.
    Every rank runs the same batches; rank 0 logs `validation {json}`.  The records are `module.val_history`.
    metrics_log: rank 0 appends one JSON object per line to this file, {"step", "split": "train", ...} for every training
    record and {"step", "split": "val", ...} for every pass."""
    import torch.distributed as dist
    rank = dist.get_rank() if dist.is_initialized() else 0
    if uncert and not cfg.VOXEL_SEG.ENABLED:
        raise ValueError('the `_uncert` panel needs the voxel head (VOXEL_SEG.ENABLED)')
    torch.manual_seed(seed)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=device)
    module.train()
    if panel_dir and rank == 0:
        from muvo_amd.visualise import PanelWriter
        module.panel_writer = PanelWriter(panel_dir)
        module.traj_panels = bool(traj)
        module.traj_options = dict(traj_options or {})
        module.flow_panels = bool(flow)
        module.voxel_panels = bool(voxel)
        module.voxel_options = dict(size=int(voxel_size))
        module.inst_panels = bool(inst)
        module.uncert_panels = bool(uncert)
    if setup is not None:
        setup(module)
    opts, scheds = module.configure_optimizers()
    optimizer, scheduler = opts[0], scheds[0]['scheduler']
    torch.manual_seed(seed + 7919 * rank)         # data-dependent randomness (RSSM noise, augmentation) differs per rank
    global_step = load_checkpoint(module, optimizer, scheduler, resume) if resume else 0
    module._global_step = global_step
    steps = cfg.STEPS if steps is None else steps
    accum = max(1, int(cfg.OPTIMIZER.ACCUMULATE_GRAD_BATCHES))
    s = cfg.RECEPTIVE_FIELD + cfg.FUTURE_HORIZON
    world = dist.get_world_size() if dist.is_initialized() else 1
    history, micro = [], global_step * accum
    dataset_root = dataset_root or cfg.DATASET.DATAROOT
    data = None
    if dataset_root and batch_fn is None:
        from muvo_amd.data.dataset import DataModule
        data = DataModule(cfg, dataset_root, device=device, rank=rank, world_size=world, seed=seed, input_stream=input_stream)
        data.setup()
        recorded = data.train_batches(start=micro)        # a resumed run continues the order of the interrupted one
        batch_fn = lambda _micro: next(recorded)          # noqa: E731
    module.val_history = []
    metrics_file = None
    if metrics_log and rank == 0:
        from muvo_amd.validate import JsonLines
        metrics_file = JsonLines(metrics_log)
    if validate:
        from muvo_amd import validate as V
        say = (log or print) if rank == 0 else (lambda line: None)
        if val_batch_fn is not None:
            val_loaders = lambda: [val_batch_fn(idx) for idx in range(3)]         # noqa: E731
        elif data is not None:
            recorded_val = data.val_dataloader()          # made once: every pass iterates them from their start, in the same slots
            val_loaders = lambda: recorded_val            # noqa: E731
        else:
            val_loaders = lambda: [V.SyntheticLoader(cfg, max(limit_val_batches, sanity_val_steps), seed, device)]   # noqa: E731
        if not resume and sanity_val_steps > 0:
            sanity = V.run_validation(module, val_loaders(), limit_batches=sanity_val_steps, seed=seed, panels=False)
            say(f'sanity validation: {json.dumps(V.jsonable(sanity)["batches"])}')
    t0 = time.time()
    while global_step < steps:
        # every optimizer step starts from its own seed: a resumed run draws the same RSSM noise / augmentation as the
        # uninterrupted one (the dropout seeds already depend on (rank, optimizer step, micro-batch) only)
        torch.manual_seed(seed + 7919 * rank + 104729 * (global_step + 1))
        optimizer.zero_grad()
        for k in range(accum):
            module.accumulate_now = k < accum - 1
            batch = batch_fn(micro) if batch_fn else make_batch(cfg.BATCHSIZE, s, seed=seed + micro * world + rank, device=device)
            loss = module.training_step(batch, micro)
            (loss / accum if accum > 1 else loss).backward()      # Lightning divides the loss by accumulate_grad_batches
            module.on_after_backward()
            micro += 1
        optimizer.step()
        scheduler.step()
        global_step += 1
        module._global_step = global_step
        if log is not None or global_step % max(1, cfg.LOGGING_INTERVAL) == 0 or global_step == steps:
            rec = {k: float(v.detach()) for k, v in module.logged.items()}
            rec['step'], rec['lr'] = global_step, optimizer.param_groups[0]['lr']
            history.append(rec)
            if rank == 0:
                total = sum(v for k, v in rec.items() if k.startswith('train_'))
                line = json.dumps({'step': global_step, 'loss': total, 'lr': rec['lr'], 's_per_step': (time.time() - t0) / len(history)})
                (log or print)(line)
                if metrics_file is not None:
                    metrics_file.write(global_step, 'train', rec)
        if cfg.VAL_CHECK_INTERVAL and global_step % cfg.VAL_CHECK_INTERVAL == 0 and rank == 0:
            name = save_checkpoint(module, optimizer, scheduler, global_step, cfg.LOG_DIR)
            (log or print)(f'checkpoint {name}')
        if validate and V.validates_at(global_step, cfg.VAL_CHECK_INTERVAL):
            # after the checkpoint (Lightning: ModelCheckpoint.on_train_batch_end, then the validation loop): the file of step k
            # holds what this pass runs on, but for the BatchNorm running buffers, which validation moves (trainer.py:405)
            tv = time.time()
            result = V.run_validation(module, val_loaders(), limit_batches=limit_val_batches, seed=seed)
            record = {'step': global_step, **result}          # (the pass ends with the read of its sums: the device is idle)
            module.val_history.append(record)
            line = {**V.jsonable(record), 's_per_pass': time.time() - tv}
            say('validation ' + json.dumps(line))
            if metrics_file is not None:
                metrics_file.write(global_step, 'val', line)
            t0 += time.time() - tv                # s_per_step of the training lines stays the training loop's
    return module, history


def build_parser():
    parser = get_parser()
    parser.add_argument('--resume', default='', help='Lightning-format checkpoint to continue from')
    parser.add_argument('--dataset-root', default='', help='directory of recorded runs (overrides DATASET.DATAROOT)')
    parser.add_argument('--panel-dir', default='', metavar='DIR', help='write the picture grids of every LOG_VIDEO_INTERVAL-th step here (rank 0)')
    parser.add_argument('--traj', action='store_true', help='with --panel-dir: also the ego-trajectory panel `_traj` (ICP between lidar frames)')
    parser.add_argument('--flow', action='store_true', help='with --panel-dir: also the optical-flow panel `_flow` (dense Farneback flow between camera frames)')
    parser.add_argument('--voxel', action='store_true', help='with --panel-dir: also the 3-D voxel panel `_voxel` (the grids ray-cast on the device)')
    parser.add_argument('--inst', action='store_true', help='with --panel-dir: also the BEV instance panel `_inst` (label ids and the ids decoded from the centre / offset heads)')
    parser.add_argument('--uncert', action='store_true', help='with --panel-dir: also the uncertainty panel `_uncert` (top views of the voxel head\'s predictive entropy and mutual information)')
    parser.add_argument('--voxel-size', type=int, default=256, metavar='R', help='--voxel: pixels a side of one tile (default 256)')
    parser.add_argument('--traj-stride', type=int, default=4, metavar='K', help='--traj: every K-th source point is an ICP query (default 4; 1 = exact)')
    parser.add_argument('--traj-max-iteration', type=int, default=200, metavar='N', help='--traj: ICP iteration cap (default 200; the reference: 2000)')
    parser.add_argument('--traj-search', choices=('brute', 'grid'), default='brute',
                        help='--traj: neighbour search of the ICP (default brute; grid: a cell grid of the target points, the same result bit for bit)')
    parser.add_argument('--validate', action='store_true',
                        help='validate every VAL_CHECK_INTERVAL steps (after that step\'s checkpoint), with a sanity pass before the first step')
    parser.add_argument('--limit-val-batches', type=int, default=3, metavar='N', help='batches per validation loader and pass (default 3)')
    parser.add_argument('--sanity-val-steps', type=int, default=2, metavar='N', help='batches per loader of the sanity pass (default 2; 0: none)')
    parser.add_argument('--metrics-log', default='', metavar='FILE', help='append the training and validation records here, one JSON object per line (rank 0)')
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    cfg = get_cfg(args)
    import torch.distributed as dist
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local_rank)
    device = torch.device('cuda', local_rank)
    if world > 1:
        dist.init_process_group('nccl', device_id=device)
    fit(cfg, device, resume=args.resume or None, dataset_root=args.dataset_root or None, panel_dir=args.panel_dir or None, traj=args.traj,
        traj_options=dict(source_stride=args.traj_stride, max_iteration=args.traj_max_iteration, search=args.traj_search),
        validate=args.validate, limit_val_batches=args.limit_val_batches, sanity_val_steps=args.sanity_val_steps,
        metrics_log=args.metrics_log or None, flow=args.flow, voxel=args.voxel, voxel_size=args.voxel_size, inst=args.inst, uncert=args.uncert)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    sys.exit(main())
