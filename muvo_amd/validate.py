"""Validation: what Lightning's validation loop does with the reference's module (train.py:104-110: `limit_val_batches = 3`,
`num_sanity_val_steps = 2`, a pass every `VAL_CHECK_INTERVAL` optimizer steps) - `validation_step` over the first batches of
every validation loader, then `on_validation_epoch_end` - as one routine that `muvo_amd.train.fit` calls between two optimizer
steps and that this command line runs on a checkpoint.  One process, one GPU.

    python -m muvo_amd.validate --config-file muvo_amd/configs/test_base_1d.yml --dataset-root /data/carla \\
        --checkpoint epoch=0-step=50000.ckpt [--limit-batches 3] [--out runs/val]

writes `OUT/val_metrics.json`: the result of `run_validation` over `DataModule.val_dataloader()`.

A pass depends on the weights, the batches, the seed and one switch only: batch i of loader idx starts from seeds that are a
function of (seed, idx, i) (`predict.seed_batch`: torch, numpy, the model's dropout counters), the Chamfer subset is drawn from
that numpy seed and handed over explicitly.  The curve of a run is therefore the same batches under the same noise at every
pass, and a pass of `fit` at step k equals the pass of this tool over the checkpoint of step k.  The switch is
`model.rssm.active_inference`: `training_step` throws it at micro-batch number STEPS (trainer.py:394-399), from then on the
imagination takes its actions from the policy (transition.py:151-173) and the RSSM leaves its fused kernel; it is module state
that no checkpoint carries, in the reference as here.  `--active-inference` sets it for a pass over a checkpoint written after
that point."""
import json
import os
import sys

import numpy as np
import torch

from muvo_amd.config import get_cfg, get_parser

CD_POINTS = 10000                                     # trainer.py:455: the size of the Chamfer subset


def refuse_multi_process(environ=None):
    environ = os.environ if environ is None else environ
    world = int(environ.get('WORLD_SIZE', '1') or 1)
    if world > 1:
        raise RuntimeError(f'muvo_amd.validate runs in one process on one GPU (WORLD_SIZE={world}): start it without a launcher; '
                           'validation next to a multi-process training run is `muvo_amd.train --validate`')


def validation_steps(interval, steps, resume_step=0):
    """The optimizer steps after which a run of `steps` steps validates: the multiples of `interval` (VAL_CHECK_INTERVAL; the
    reference's `val_check_interval = VAL_CHECK_INTERVAL * ACCUMULATE_GRAD_BATCHES` counts micro-batches) above the step a
    resumed run starts from.  interval 0: none."""
    interval, steps, resume_step = int(interval or 0), int(steps), int(resume_step)
    if interval <= 0:
        return []
    return [k for k in range(interval, steps + 1, interval) if k > resume_step]


def validates_at(step, interval):
    return bool(interval) and int(interval) > 0 and step > 0 and step % int(interval) == 0


class EpochMean:
    """Lightning's epoch mean of what a validation step logs: per name the sum over the batches, kept where the values are
    (float64: the sum of a few float32 numbers is then exact to the last bit of the mean) and read with ONE copy in `result`."""

    def __init__(self):
        self.names, self.total, self.count = None, None, 0

    def add(self, values):
        """values: {name: 0-d tensor}; every call brings the same names."""
        names = list(values)
        if self.names is None:
            self.names = names
        elif names != self.names:
            raise ValueError(f'EpochMean: names changed between batches: {sorted(set(names) ^ set(self.names))}')
        if names:
            row = torch.stack([values[n].detach().reshape(()) for n in names]).double()
            self.total = row if self.total is None else self.total + row
        self.count += 1

    def result(self):
        if not self.names or not self.count:
            return {}
        return dict(zip(self.names, (self.total / self.count).tolist()))


class JsonLines:
    """One JSON object per line, appended: {"step": k, "split": "train" | "val", ...}."""

    def __init__(self, path):
        self.path = path
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)

    def write(self, step, split, record):
        row = {'step': int(step), 'split': split}
        row.update({k: v for k, v in record.items() if k not in row})
        with open(self.path, 'a') as fh:
            fh.write(json.dumps(row) + '\n')
        return row

    @staticmethod
    def read(path):
        with open(path) as fh:
            return [json.loads(line) for line in fh if line.strip()]


def _rng_state(device):
    state = {'numpy': np.random.get_state(), 'torch': torch.get_rng_state()}
    if device is not None and device.type == 'cuda':
        state['device'] = torch.cuda.get_rng_state(device)
    return state


def _set_rng_state(state, device):
    np.random.set_state(state['numpy'])
    torch.set_rng_state(state['torch'])
    if 'device' in state:
        torch.cuda.set_rng_state(state['device'], device)


def _reset_metric_sets(module):
    """Every accumulator of the validation metric sets back to empty (an interrupted or discarded pass)."""
    for sets in (module.metrics_vals, module.metrics_vals_imagine):
        for metrics in sets:
            for metric in metrics.values():
                metric.reset()


def _n_points(cfg, batch):
    """The number of range-view points per frame the Chamfer subset is drawn from (trainer.py:453-455)."""
    rv = batch.get('range_view_pcd_xyzd')
    if rv is None:
        rv = batch['range_view_label_1']
    return int(rv.shape[-2]) * int(rv.shape[-1])


def run_validation(module, loaders, limit_batches=3, seed=1234, log=None, panels=True, drop_sensor=None):
    """One validation pass: for every loader idx of `loaders` (a list of iterables of device batches; an empty one is skipped and
    contributes no names) `module.validation_step` over its first `limit_batches` batches, then `on_validation_epoch_end`.

    Returns {name: float} with every name of metric_names(cfg, 'val{idx}') and metric_names(cfg, 'val_imagine{idx}') for the
    loaders that had batches (with an IoU head also `..._confusion`: nested integer lists); the reference's loss curves
    `val{idx}_{term}` / `val{idx}_{term}_imagine` (first imagined sample; trainer.py:495-499) and the totals `val{idx}_loss` /
    `val{idx}_loss_imagine` as means over the pass's batches - summed on the device, read once at the end; and
    `batches`: {idx: number of batches}.  Nothing lands in `module.logged`.  panels=False: nothing is drawn even when the module
    has a `panel_writer` (the sanity pass).

    drop_sensor: 'camera' or 'lidar' - every batch runs without that sensor (muvo_amd.predict.set_sensor_drop); the result gains
    the entry `drop_sensor`.

    `model.rssm.active_inference` is read as it stands (the module docstring), like the weights.

    The module is left as it was found, also when a step raises: the `training` flags, `model.seed_epoch` and
    `model._step_seed`, the numpy RNG and the torch RNGs (CPU and the module's device), `log_fn`, `on_confusion`, `panel_writer`,
    `vis_step`; the validation metric sets are reset.  NOT restored: the BatchNorm running statistics.  The reference validates
    with `self.train()` (trainer.py:405), so its running buffers move during validation, and `_eval_step` reproduces that."""
    from muvo_amd import ops
    from muvo_amd.predict import seed_batch, set_sensor_drop
    model = module.model
    device = next(model.parameters()).device
    was_training = [(m, m.training) for m in module.modules()]
    was_seeds = (model.seed_epoch, model._step_seed)
    was_rng = _rng_state(device)
    was_hooks = (module.log_fn, module.on_confusion, module.panel_writer, module.vis_step)
    logged, confusion, counts, means = {}, {}, {}, {}
    sink = lambda name, value: None                                     # noqa: E731
    done = False
    try:
        module.log_fn = sink                      # validation_step's own `self.log` calls (panels on): the means below carry them
        if not panels:
            module.panel_writer = None
        for idx, loader in enumerate(loaders):
            if loader is None:
                continue
            n, it = 0, iter(loader)
            try:
                while n < limit_batches:
                    try:
                        batch = next(it)
                    except StopIteration:
                        break
                    batch = set_sensor_drop(module.cfg, dict(batch), drop_sensor)   # a copy: preprocess adds the label pyramids to the dict it is given
                    seed_batch(module, seed, idx, n)
                    cd_index =np.random.randint(0, _n_points(module.cfg, batch), CD_POINTS) if module.cfg.LIDAR_RE.ENABLED else None
                    out, loss, _, loss_imagines, _ = module.validation_step(batch, n, idx, cd_index=cd_index)
                    values = {f'val{idx}_{k}': v for k, v in loss.items()}
                    if loss_imagines:
                        values.update({f'val{idx}_{k}_imagine': v for k, v in loss_imagines[0].items()})
                    values.update(out)
                    means.setdefault(idx, EpochMean()).add(values)
                    n += 1
            finally:
                close = getattr(it, 'close', None)        # a loader left before its end: its reader threads end here, not at a
                if close is not None:                     # later garbage collection
                    close()
            if n:
                counts[idx] = n
        module.log_fn = lambda name, value: logged.__setitem__(name, float(value))
        module.on_confusion = lambda name, matrix: confusion.__setitem__(name, matrix.tolist())
        module.on_validation_epoch_end()
        done = True
    finally:
        module.log_fn, module.on_confusion, module.panel_writer, module.vis_step = was_hooks
        if not done:
            _reset_metric_sets(module)
            ops.reset_accumulators()
        for m, flag in was_training:
            m.training = flag
        model.seed_epoch, model._step_seed = was_seeds
        _set_rng_state(was_rng, device)
    result = {**logged, **confusion}
    for idx in counts:
        result.update(means[idx].result())
    result['batches'] = counts
    if drop_sensor is not None:
        result['drop_sensor'] = drop_sensor
    if log is not None:
        log(json.dumps(jsonable(result)))
    return result


def jsonable(result):
    return {k: ({str(i): n for i, n in v.items()} if k == 'batches' else v) for k, v in result.items()}


class SyntheticLoader:
    """`n` synthetic validation batches, made again at every pass; their seeds are negative, those of the training batches
    (seed + micro-batch number) are not."""

    def __init__(self, cfg, n, seed, device):
        self.cfg, self.n, self.seed, self.device = cfg, int(n), int(seed), device

    def __iter__(self):
        from muvo_amd.data.synthetic import make_batch
        s = self.cfg.RECEPTIVE_FIELD + self.cfg.FUTURE_HORIZON
        for i in range(self.n):
            yield make_batch(self.cfg.BATCHSIZE, s, seed=-(1 + abs(self.seed) + i), device=self.device)


def build_parser():
    parser = get_parser()
    parser.description = 'One validation pass of a checkpoint over the validation loaders of recorded runs'
    parser.add_argument('--dataset-root', default='', help='directory of recorded runs (overrides DATASET.DATAROOT)')
    parser.add_argument('--checkpoint', default='', help='Lightning-format checkpoint (goes to PRETRAINED.PATH)')
    parser.add_argument('--limit-batches', type=int, default=3, metavar='N', help='at most N batches per loader (default 3)')
    parser.add_argument('--out', default='.', metavar='DIR', help='directory for val_metrics.json (default: the current one)')
    parser.add_argument('--seed', type=int, default=1234)
    parser.add_argument('--drop-sensor', choices=('camera', 'lidar'), default=None,
                        help='every sample runs without that sensor (as python -m muvo_amd.predict --drop-sensor); val_metrics.json '
                             'gains a "drop_sensor" entry')
    parser.add_argument('--active-inference', action='store_true',
                        help='set model.rssm.active_inference: the checkpoint comes from a run that had passed micro-batch STEPS')
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    refuse_multi_process()
    if args.limit_batches < 1:
        raise SystemExit('--limit-batches must be positive')
    cfg = get_cfg(args)
    from muvo_amd.predict import check_drop_sensor
    try:
        check_drop_sensor(cfg, args.drop_sensor)
    except ValueError as e:
        raise SystemExit(str(e))
    if args.checkpoint:
        cfg.defrost()
        cfg.PRETRAINED.PATH = args.checkpoint
        cfg.freeze()
    torch.cuda.set_device(0)
    device = torch.device('cuda', 0)
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    torch.manual_seed(args.seed)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=device)
    module.model.rssm.active_inference = bool(args.active_inference)
    data = DataModule(cfg, args.dataset_root or cfg.DATASET.DATAROOT, device=device, seed=args.seed)
    data.setup()
    result = jsonable(run_validation(module, data.val_dataloader(), limit_batches=args.limit_batches, seed=args.seed,
                                     drop_sensor=args.drop_sensor))
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, 'val_metrics.json')
    with open(path, 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps({'written': path, 'batches': result['batches']}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
