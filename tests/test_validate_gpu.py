"""-m gpu: validation inside `muvo_amd.train.fit` (the reference's train.py:104-110 under Lightning: sanity pass, a pass every
VAL_CHECK_INTERVAL steps after that step's checkpoint, three batches per loader) and `muvo_amd.validate.run_validation`.
Smallest sizes at which the loop can go wrong: 2 observed + 1 imagined frame, batch 1, 4 steps with a pass after steps 2 and 4,
4 validation batches so the limit of 3 bites.  Deterministic mode throughout: equal means equal.  One run with and one
without validation serve the first three tests.

An optimizer step is 2 micro-batches here, not base_1d's 16 (OPTIMIZER.ACCUMULATE_GRAD_BATCHES): a micro-batch takes half a
second in deterministic mode, and the two 4-step runs would take 70 s instead of 9.  Two is the smallest count at which a step
still accumulates (`accumulate_now`, the dropout seed counter within a step), and it puts micro-batch number STEPS = 4, where
`training_step` switches the RSSM to active inference (trainer.py:394-399), between the two passes: the pass after step 2
runs with the switch off, the one after step 4 with it on."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 1234
EXTRA = ('step', 'batches')
ACCUMULATE = 2


def _cfg(**kw):
    from muvo_amd.config import base_1d_cfg
    base = dict(RECEPTIVE_FIELD=2, FUTURE_HORIZON=1, BATCHSIZE=1, STEPS=4, VAL_CHECK_INTERVAL=2, LOGGING_INTERVAL=1,
                OPTIMIZER__ACCUMULATE_GRAD_BATCHES=ACCUMULATE)
    base.update(kw)
    return base_1d_cfg(**base)


def _loss_names(history, idx=0):
    """The loss curves of one loader from the terms the training step logs: all of them for the reconstruction, all but the KL
    term - an imagined roll-out has no posterior - for the imagination, and the two totals."""
    terms = [k[len('train_'):] for k in history[0] if k.startswith('train_')]
    assert len(terms) == 21 and 'probabilistic' in terms
    return ([f'val{idx}_{t}' for t in terms] + [f'val{idx}_{t}_imagine' for t in terms if t != 'probabilistic']
            + [f'val{idx}_loss', f'val{idx}_loss_imagine'])


def _state(module):
    params = {n: p.detach().clone() for n, p in module.model.named_parameters()}
    return params, module.store.exp_avg.clone(), module.store.exp_avg_sq.clone()


@pytest.fixture(scope='module')
def world(dev, tmp_path_factory):
    from muvo_amd import ops, train
    from muvo_amd.data.synthetic import make_batch
    cfg = _cfg()
    assert cfg.PREDICTION.N_SAMPLES >= 1
    val_batches = [make_batch(1, 3, seed=-(1 + k), device=dev) for k in range(4)]
    assert cfg.OPTIMIZER.ACCUMULATE_GRAD_BATCHES == ACCUMULATE
    train_batches = [make_batch(1, 3, seed=SEED + k, device=dev) for k in range(4)]     # made once, served in turn
    batch_fn = lambda micro: dict(train_batches[micro % len(train_batches)])      # noqa: E731
    drawn = []

    def val_batch_fn(idx):
        if idx != 0:
            return None

        def gen():
            for k, b in enumerate(val_batches):
                drawn.append(k)
                yield dict(b)
        return gen()

    w = types.SimpleNamespace(cfg=cfg, val_batches=val_batches, val_batch_fn=val_batch_fn, drawn=drawn)
    was, cwd = ops.get_deterministic(), os.getcwd()
    ops.set_deterministic(True)
    try:
        # transformer dropout stays ON in both runs: its seed counters are among what validation must put back
        w.dir_val = str(tmp_path_factory.mktemp('with_validation'))
        os.chdir(w.dir_val)
        w.lines = []
        w.module, w.history = train.fit(cfg, dev, log=w.lines.append, batch_fn=batch_fn, validate=True, val_batch_fn=val_batch_fn,
                                        metrics_log=os.path.join(w.dir_val, 'log', 'metrics.jsonl'))
        w.state = _state(w.module)
        w.drawn_by_fit = list(drawn)
        w.dir_plain = str(tmp_path_factory.mktemp('plain'))
        os.chdir(w.dir_plain)
        w.lines_plain = []
        w.module_plain, w.history_plain = train.fit(cfg, dev, log=w.lines_plain.append, batch_fn=batch_fn)
        w.state_plain = _state(w.module_plain)
        os.chdir(cwd)
        yield w
    finally:
        os.chdir(cwd)
        ops.set_deterministic(was)


def test_fit_validates(world):
    from muvo_amd.trainer import metric_names
    from muvo_amd.validate import JsonLines
    w, cfg = world, world.cfg
    for l in w.lines:
        print(l[:120], '...', l[-48:])
    assert w.lines.count('sanity validation: {"0": 2}') == 1 and w.lines.index('sanity validation: {"0": 2}') == 0
    # the sanity pass drew batches 0, 1 and looked no further; every pass drew 0, 1, 2 from a loader started afresh
    assert w.drawn_by_fit == [0, 1, 0, 1, 2, 0, 1, 2]
    logged = [json.loads(l[len('validation '):]) for l in w.lines if l.startswith('validation ')]
    records = w.module.val_history
    assert [r['step'] for r in logged] == [r['step'] for r in records] == [2, 4]
    names = metric_names(cfg, 'val0') + metric_names(cfg, 'val_imagine0') + _loss_names(w.history)
    assert len(set(names)) == len(names) == 2 * 9 + 21 + 20 + 2
    for rec, line in zip(records, logged):
        assert sorted(rec) == sorted(names + list(EXTRA))
        assert rec['batches'] == {0: 3} and line['batches'] == {'0': 3}
        for n in names:
            print(rec['step'], n, rec[n])
            assert isinstance(rec[n], float) and np.isfinite(rec[n]), (n, rec[n])
            assert line[n] == rec[n]
        assert line['s_per_pass'] > 0
    assert records[0] != records[1]                                   # two optimizer steps lie between the passes
    # the order of the lines: step 2's record, its checkpoint, its validation
    order = [l.split(' ')[0] if not l.startswith('{') else 'step' for l in w.lines]
    assert order == ['sanity'] + ['step', 'step', 'checkpoint', 'validation'] * 2
    # the training history is what a run without validation records: no val* name reached module.logged
    assert [sorted(h) for h in w.history] == [sorted(h) for h in w.history_plain]
    assert not any(k.startswith('val') for k in w.module.logged)
    ckpts = ['epoch=0-step=2.ckpt', 'epoch=0-step=4.ckpt']
    assert sorted(f for f in os.listdir(w.dir_val) if f.endswith('.ckpt')) == ckpts
    assert sorted(f for f in os.listdir(w.dir_plain) if f.endswith('.ckpt')) == ckpts
    # the metric log: every training record and every pass, in the order they happened
    rows = JsonLines.read(os.path.join(w.dir_val, 'log', 'metrics.jsonl'))
    assert [(r['step'], r['split']) for r in rows] == [(1, 'train'), (2, 'train'), (2, 'val'), (3, 'train'), (4, 'train'), (4, 'val')]
    assert {k: v for k, v in rows[0].items() if k != 'split'} == w.history[0]
    assert {k: v for k, v in rows[2].items() if k != 'split'} == logged[0]
    # the run without validation logs what it always did
    assert not any(l.startswith(('validation', 'sanity')) for l in w.lines_plain)
    assert w.module_plain.val_history == []


def test_validation_does_not_move_training(world):
    """Same configuration, dropout on, with and without validation: after 4 steps the parameters, both AdamW moments and the
    training losses of every step are bit-identical.  Left out: the BatchNorm running buffers (not parameters), which the
    reference's validation moves as well (trainer.py:405), and nothing else."""
    w = world
    assert any(layer.p > 0 for layer in w.module.model.transformer_encoder.layers)
    params, m, v = w.state
    params_plain, m_plain, v_plain = w.state_plain
    assert list(params) == list(params_plain) and len(params) > 400
    moved = [n for n in params if not torch.equal(params[n], params_plain[n])]
    assert moved == [], (len(moved), moved[:8])
    assert torch.equal(m, m_plain) and torch.equal(v, v_plain) and float(m.abs().sum()) > 0
    assert [h['step'] for h in w.history] == [h['step'] for h in w.history_plain] == [1, 2, 3, 4]
    for a, b in zip(w.history, w.history_plain):
        keys = [k for k in a if k.startswith('train_')]
        assert len(keys) == 21
        for k in keys + ['lr', '-global_step']:
            assert a[k] == b[k], (a['step'], k, a[k], b[k])
    # (validation did run in between: the running statistics differ)
    bufs, bufs_plain = dict(w.module.model.named_buffers()), dict(w.module_plain.model.named_buffers())
    assert any(not torch.equal(bufs[n], bufs_plain[n]) for n in bufs if n.endswith('running_mean'))


@pytest.fixture(scope='module')
def from_checkpoint(dev, world):
    """A module of its own with the weights of step 2's checkpoint, as `python -m muvo_amd.validate --checkpoint` builds it."""
    from muvo_amd.trainer import WorldModelTrainer
    return WorldModelTrainer(world.cfg.convert_to_dict(), pretrained_path=os.path.join(world.dir_val, 'epoch=0-step=2.ckpt'), device=dev)


def test_pass_equals_the_pass_over_its_checkpoint(world, from_checkpoint):
    """The checkpoint of step 2 is written before step 2's validation, and a pass depends on nothing but weights, batches and
    seed: a fresh module with that file's weights gives the record of step 2, every value bit-identical."""
    from muvo_amd import ops
    from muvo_amd.validate import run_validation
    w = world
    assert from_checkpoint.model.rssm.active_inference is False
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        got = run_validation(from_checkpoint, [w.val_batch_fn(0)], limit_batches=3, seed=SEED)
    finally:
        ops.set_deterministic(was)
    want = {k: v for k, v in w.module.val_history[0].items() if k != 'step'}
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert diff == {}
    # ... and differs from the pass two optimizer steps later
    assert got['val0_loss'] != w.module.val_history[1]['val0_loss']


def test_pass_after_the_active_inference_switch(dev, world):
    """Between the two passes `training_step` has switched the RSSM to active inference (micro-batch number STEPS): module state
    that no checkpoint carries, in the reference as here.  Handed over, as `python -m muvo_amd.validate --active-inference`
    does, the pass over the checkpoint of step 4 is the record of step 4 bit for bit; left off, the imagination differs."""
    from muvo_amd import ops
    from muvo_amd.trainer import WorldModelTrainer
    from muvo_amd.validate import run_validation
    w = world
    assert w.module.model.rssm.active_inference is True
    fresh = WorldModelTrainer(w.cfg.convert_to_dict(), pretrained_path=os.path.join(w.dir_val, 'epoch=0-step=4.ckpt'), device=dev)
    want = {k: v for k, v in w.module.val_history[1].items() if k != 'step'}
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        off = run_validation(fresh, [w.val_batch_fn(0)], limit_batches=3, seed=SEED)
        fresh.model.rssm.active_inference = True
        on = run_validation(fresh, [w.val_batch_fn(0)], limit_batches=3, seed=SEED)
    finally:
        ops.set_deterministic(was)
    assert {k: (on[k], want[k]) for k in want if on[k] != want[k]} == {}
    assert off['val0_steering_imagine'] != want['val0_steering_imagine'] and off['val0_loss_imagine'] != want['val0_loss_imagine']


def _snapshot(module):
    return dict(training=[m.training for m in module.modules()], seeds=(module.model.seed_epoch, module.model._step_seed),
                numpy=np.random.get_state(), torch=torch.get_rng_state(), device=torch.cuda.get_rng_state(),
                hooks=(module.log_fn, module.on_confusion, module.panel_writer, module.vis_step), logged=dict(module.logged))


def _same(a, b):
    assert a['training'] == b['training'] and a['seeds'] == b['seeds']
    assert a['numpy'][0] == b['numpy'][0] and np.array_equal(a['numpy'][1], b['numpy'][1]) and a['numpy'][2:] == b['numpy'][2:]
    assert torch.equal(a['torch'], b['torch']) and torch.equal(a['device'], b['device'])
    assert all(x is y for x, y in zip(a['hooks'][:3], b['hooks'][:3])) and a['hooks'][3] == b['hooks'][3]
    assert list(a['logged']) == list(b['logged']) and all(a['logged'][k] is b['logged'][k] for k in a['logged'])


def test_restore(dev, world, from_checkpoint):
    from muvo_amd import ops
    from muvo_amd.validate import run_validation
    w, module = world, from_checkpoint
    module.train()
    module.model.transformer_encoder.layers[0].eval()                  # a flag that differs from its neighbours comes back too
    module.model.seed_epoch, module.model._step_seed = 5, 7
    log_fn, on_confusion = (lambda name, value: None), (lambda name, matrix: None)
    module.log_fn, module.on_confusion, module.panel_writer, module.vis_step = log_fn, on_confusion, None, 41
    module.logged = {'train_rgb_1': torch.ones((), device=dev)}
    torch.manual_seed(99)
    np.random.seed(99)
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        before = _snapshot(module)
        clean = run_validation(module, [w.val_batch_fn(0)], limit_batches=3, seed=SEED)
        _same(before, _snapshot(module))
        assert clean['batches'] == {0: 3}
        # the numpy and torch streams go on as if nothing had happened
        np_next, torch_next = np.random.randint(0, 2 ** 31), torch.rand(3)
        np.random.seed(99)
        torch.manual_seed(99)
        assert np_next == np.random.randint(0, 2 ** 31) and torch.equal(torch_next, torch.rand(3))

        def broken():
            for k, b in enumerate(w.val_batches):
                b = dict(b)
                if k == 1:
                    del b['image']
                yield b
        before = _snapshot(module)
        with pytest.raises(KeyError, match='image'):
            run_validation(module, [broken()], limit_batches=3, seed=SEED)
        _same(before, _snapshot(module))
        for sets in (module.metrics_vals, module.metrics_vals_imagine):            # the first batch's sums are gone
            m = sets[0]
            assert m['ssim'].count == 1e-8 and m['psnr'].count == 1e-8 and m['cd'].count == 1e-8 and m['ssc'].count == 1e-8
            assert int(m['ssc'].tps.sum()) == 0
        again = run_validation(module, [w.val_batch_fn(0)], limit_batches=3, seed=SEED)
        assert again == clean
    finally:
        ops.set_deterministic(was)
        module.log_fn = module.on_confusion = None
        module.logged = {}
        module.train()


def test_recorded_runs(dev, tmp_path, monkeypatch):
    """Validation batches from `DataModule.val_dataloader()`: val0 has four batches (12 frames, sequences of 3 frames 0.2 s
    apart from 0.2 s on: 4 sequences, sampler step 1), val1 / val2 have none and contribute no names."""
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd import ops, train
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import metric_names
    root = str(tmp_path / 'rec')
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 9, True), ('val0', 'Town02', '0000', 12, True)))
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=1, BATCHSIZE=1, STEPS=4, VAL_CHECK_INTERVAL=2, LOGGING_INTERVAL=1,
                           OPTIMIZER__ACCUMULATE_GRAD_BATCHES=ACCUMULATE)
    monkeypatch.setattr(DataModule, 'VAL', (('val0', 0, 1), ('val1', 1500, 50), ('val2', 3000, 50)))
    dm = DataModule(cfg, root, device=dev, seed=SEED)
    dm.setup()
    assert [len(l) for l in dm.val_dataloader()] == [4, 0, 0] and len(dm.train_dataset) == 1
    monkeypatch.chdir(tmp_path)
    panel_dir = tmp_path / 'panels'
    lines = []
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        module, history = train.fit(cfg, dev, steps=2, log=lines.append, dataset_root=root, validate=True, panel_dir=str(panel_dir))
        # the command line over the checkpoint of step 2 (the same configuration as file + options) repeats step 2's pass
        from muvo_amd import config, validate
        opts = ['RECEPTIVE_FIELD', '2', 'FUTURE_HORIZON', '1', 'BATCHSIZE', '1', 'STEPS', '4', 'VAL_CHECK_INTERVAL', '2',
                'LOGGING_INTERVAL', '1', 'OPTIMIZER.ACCUMULATE_GRAD_BATCHES', str(ACCUMULATE)]
        for k, v in RI.CFG_OVERRIDES.items():
            opts += [k, str(v)]
        config_file = os.path.join(os.path.dirname(config.__file__), 'configs', 'test_base_1d.yml')
        assert validate.main(['--config-file', config_file, '--dataset-root', root, '--checkpoint', 'epoch=0-step=2.ckpt',
                              '--out', str(tmp_path / 'val')] + opts) == 0
    finally:
        ops.set_deterministic(was)
    assert lines[0] == 'sanity validation: {"0": 2}'
    assert [l.split(' ')[0] for l in lines if not l.startswith('{')] == ['sanity', 'checkpoint', 'validation']
    (record,) = module.val_history
    names = metric_names(cfg, 'val0') + metric_names(cfg, 'val_imagine0') + _loss_names(history)
    assert sorted(record) == sorted(names + list(EXTRA)) and record['step'] == 2 and record['batches'] == {0: 3}
    assert not any(k.startswith(('val1', 'val2', 'val_imagine1', 'val_imagine2')) for k in record)
    assert all(np.isfinite(record[n]) for n in names)
    assert not any(k.startswith('val') for h in history for k in h) and [h['step'] for h in history] == [1, 2]
    assert os.listdir(tmp_path / 'val') == ['val_metrics.json']
    written = json.load(open(tmp_path / 'val' / 'val_metrics.json'))
    assert written == validate.jsonable({k: v for k, v in record.items() if k != 'step'})
    # panels: batch 0 of the pass at step 2, nothing from the sanity pass (which would carry step 0)
    folders = sorted(f for f in os.listdir(panel_dir) if f.startswith('val'))
    assert folders and all(f.startswith('val0_outputs_0') for f in folders)
    for f in folders:
        assert os.listdir(panel_dir / f) == ['step00000002_b0.png'], (f, os.listdir(panel_dir / f))
