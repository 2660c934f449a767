"""Host side of validation inside the training loop (muvo_amd/validate.py, muvo_amd/train.py): the schedule, the epoch mean,
the JSON-lines log, the command lines, and a loader that is left after its first batches."""
import json
import threading

import pytest
import torch


def test_schedule():
    from muvo_amd.validate import validates_at, validation_steps
    assert validation_steps(2, 4) == [2, 4]
    assert validation_steps(2, 5) == [2, 4]
    assert validation_steps(3, 10) == [3, 6, 9]
    assert validation_steps(5, 4) == []
    assert validation_steps(0, 100) == [] and validation_steps(None, 100) == []
    # a resumed run: the step it starts from was validated by the run that wrote the checkpoint
    assert validation_steps(2, 8, resume_step=4) == [6, 8]
    assert validation_steps(2, 8, resume_step=5) == [6, 8]
    assert validation_steps(2, 8, resume_step=8) == []
    # the loop's own test agrees with the list
    for interval, steps, start in ((2, 4, 0), (3, 10, 0), (2, 8, 5), (0, 6, 0), (7, 6, 0)):
        assert [k for k in range(start + 1, steps + 1) if validates_at(k, interval)] == validation_steps(interval, steps, start)


def test_epoch_mean_against_stack_mean():
    from muvo_amd.validate import EpochMean
    g = torch.Generator().manual_seed(5)
    names = ['val0_rgb_1', 'val0_voxel_1', 'val0_loss']
    rows = [torch.rand(len(names), generator=g) * torch.tensor([1e-3, 1.0, 1e3]) for _ in range(3)]
    acc = EpochMean()
    for row in rows:
        acc.add({n: row[j] for j, n in enumerate(names)})
    got = acc.result()
    assert list(got) == names and acc.count == 3
    # float64 sums of float32 values: the float64 mean to rounding (2^-52 per operation, three additions and a division)
    want64 = torch.stack(rows).double().mean(0)
    want32 = torch.stack(rows).mean(0)
    for j, n in enumerate(names):
        assert isinstance(got[n], float)
        assert abs(got[n] - float(want64[j])) <= 4 * 2.0 ** -52 * abs(float(want64[j])), (n, got[n], float(want64[j]))
        # and the float32 mean within that format's rounding of three additions and a division
        assert abs(got[n] - float(want32[j])) <= 4 * 2.0 ** -24 * abs(float(want32[j])), (n, got[n], float(want32[j]))
    assert EpochMean().result() == {}
    with pytest.raises(ValueError):
        acc.add({'val0_rgb_1': rows[0][0]})


def test_json_lines(tmp_path):
    from muvo_amd.validate import JsonLines, jsonable
    path = str(tmp_path / 'sub' / 'metrics.jsonl')
    log = JsonLines(path)
    train = {'step': 1, 'train_rgb_1': 0.25, 'lr': 1e-4}
    val = jsonable({'val0_ssim': 0.5, 'val0_loss': 3.0, 'batches': {0: 3}})
    log.write(1, 'train', train)
    log.write(2, 'val', val)
    JsonLines(path).write(3, 'train', {'step': 3, 'train_rgb_1': 0.125, 'lr': 2e-4})      # a second writer appends
    text = open(path).read()
    assert text.endswith('\n') and len(text.splitlines()) == 3
    rows = [json.loads(line) for line in text.splitlines()]
    assert rows == JsonLines.read(path)
    assert [r['split'] for r in rows] == ['train', 'val', 'train'] and [r['step'] for r in rows] == [1, 2, 3]
    assert rows[0] == {'split': 'train', **train}
    assert rows[1] == {'step': 2, 'split': 'val', 'val0_ssim': 0.5, 'val0_loss': 3.0, 'batches': {'0': 3}}


def test_train_parser_flags():
    from muvo_amd.train import build_parser
    args = build_parser().parse_args([])
    assert args.validate is False and args.limit_val_batches == 3 and args.sanity_val_steps == 2 and args.metrics_log == ''
    args = build_parser().parse_args(['--validate', '--limit-val-batches', '5', '--sanity-val-steps', '0', '--metrics-log', 'm.jsonl'])
    assert args.validate is True and args.limit_val_batches == 5 and args.sanity_val_steps == 0 and args.metrics_log == 'm.jsonl'


def test_fit_defaults_are_off():
    import inspect
    from muvo_amd.train import fit
    p = inspect.signature(fit).parameters
    assert p['validate'].default is False and p['limit_val_batches'].default == 3 and p['sanity_val_steps'].default == 2
    assert p['val_batch_fn'].default is None and p['metrics_log'].default is None


def test_validate_parser():
    from muvo_amd.validate import build_parser
    args = build_parser().parse_args(['--checkpoint', 'x.ckpt'])
    assert args.limit_batches == 3 and args.checkpoint == 'x.ckpt' and args.dataset_root == ''
    assert args.active_inference is False and build_parser().parse_args(['--active-inference']).active_inference is True


def test_main_refuses_more_than_one_process(tmp_path, monkeypatch):
    from muvo_amd import validate
    monkeypatch.setenv('WORLD_SIZE', '2')
    out = tmp_path / 'out'
    with pytest.raises(RuntimeError, match='WORLD_SIZE=2'):
        validate.main(['--out', str(out), '--checkpoint', 'none.ckpt'])
    assert not out.exists()


def test_synthetic_validation_seeds_are_not_training_seeds():
    """Training batch `micro` of rank r has seed `seed + micro * world + rank` >= seed; validation batches have negative ones."""
    from muvo_amd import validate
    from muvo_amd.data import synthetic
    seen = []

    def fake(b, s, seed, device):
        seen.append((b, s, seed))
        return {'seed': seed}

    class Cfg:
        RECEPTIVE_FIELD, FUTURE_HORIZON, BATCHSIZE = 2, 1, 1
    mp = pytest.MonkeyPatch()
    mp.setattr(synthetic, 'make_batch', fake)
    try:
        loader = validate.SyntheticLoader(Cfg, 3, 1234, 'cpu')
        first, second = [b['seed'] for b in loader], [b['seed'] for b in loader]
    finally:
        mp.undo()
    assert first == second == [-1235, -1236, -1237] and all(s == 3 for _, s, _ in seen)


def test_loader_left_early_drops_its_queue(monkeypatch):
    """Validation takes the first batches of a loader and leaves: closing the iterator cancels the staging task and the frame
    reads still queued, and the pool's thread ends.  One reader thread, two frames per batch: while frame 6 is being read,
    frame 7 and the staging of batch 3 wait behind it."""
    from concurrent.futures import ThreadPoolExecutor
    from muvo_amd.data import dataset as D

    started, staged, gate = [], [], threading.Event()

    class Frames:
        cfg, intrinsics, extrinsics = None, None, None
        data_pointers = [('run', [t]) for t in range(40)]

        def __len__(self):
            return len(self.data_pointers)

        def read_frame(self, run_id, t):
            started.append(t)
            if t >= 6:
                assert gate.wait(60)    # held until the consumer has left and dropped its queue
            return t

    class Loader(D.BatchLoader):
        def upload(self, host):
            return {'t': torch.tensor(host)}, None

    class Pool(ThreadPoolExecutor):
        def shutdown(self, *a, **k):    # the iterator's clean-up has run by now
            gate.set()
            return super().shutdown(*a, **k)

    def stack(frames, intr, extr):
        staged.append(frames[0])
        return frames[0]

    monkeypatch.setattr(D, 'ThreadPoolExecutor', Pool)
    monkeypatch.setattr(D, 'stack_frames', stack)
    monkeypatch.setattr(D, 'collate_raw', lambda raws, slot=None: list(raws))
    before = threading.active_count()
    it = iter(Loader(Frames(), 2, 'cpu', sampler=range(40), n_workers=1))
    assert [next(it)['t'].tolist() for _ in range(2)] == [[0, 1], [2, 3]]
    it.close()
    assert gate.is_set() and threading.active_count() == before
    assert sorted(started) in ([0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6]), started
    assert staged == [0, 1, 2, 3, 4, 5]
