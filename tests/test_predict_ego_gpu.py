"""-m gpu: `predict --mode test --ego-motion --traj --panels 1` over a tiny recording (the set-up of tests/test_predict_gpu.py):
ego_motion.json has the documented keys with finite values, one `_traj` PNG per sample is written, and metrics.json is
byte-identical to a run without the flags."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 77


def test_ego_motion_and_traj_leave_the_metrics_alone(dev, tmp_path):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd import predict as P
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    root = str(tmp_path / 'rec')
    os.makedirs(root)
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1, STEPS=100000)
    torch.manual_seed(SEED)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    assert module.traj_panels is False and cfg.LIDAR_RE.ENABLED

    def data():
        dm = DataModule(cfg, root, device=dev, seed=SEED)
        dm.setup()
        dm.test_sampler_0 = range(0, 4, 2)
        return dm
    a, b = str(tmp_path / 'plain'), str(tmp_path / 'ego')
    from muvo_amd import ops
    was = ops.get_deterministic()
    ops.set_deterministic(True)                             # no order-dependent float atomics in the forward pass: equal means equal
    try:
        _both_runs(P, cfg, dev, a, b, data, module)
    finally:
        ops.set_deterministic(was)


def _both_runs(P, cfg, dev, a, b, data, module):
    from muvo_amd.odometry import EgoMotionMetric
    from muvo_amd.visualise import png_read
    P.run(cfg, dev, a, 'test', loaders=[0], limit_batches=2, seed=SEED, data=data(), module=module, log=lambda s: None)
    # an untrained head: cap the iterations and thin the queries, the knobs the command line offers
    seen = {}

    def hook(i, batch, output, output_imagines):
        if i == 0:
            seen.update(batch=batch, output=output, options=dict(module.traj_options), rows=len(output_imagines))
    knobs = dict(threshold=5.0, source_stride=16, max_iteration=20)
    out = P.run(cfg, dev, b, 'test', loaders=[0], limit_batches=2, seed=SEED, data=data(), module=module, log=lambda s: None, panels=1,
                traj=True, ego_motion=dict(threshold=5.0, stride=16, max_iteration=20), icp_options=knobs, hook=hook)
    assert seen['options'] == knobs
    assert open(os.path.join(a, 'metrics.json'), 'rb').read() == open(os.path.join(b, 'metrics.json'), 'rb').read()
    assert module.traj_panels is False and module.traj_options == {} and module.panel_writer is None
    ego = json.load(open(os.path.join(b, 'ego_motion.json')))
    assert list(ego) == ['0'] and set(ego['0']) == set(EgoMotionMetric.KEYS)
    assert all(math.isfinite(v) and v >= 0 for v in ego['0'].values()), ego
    s, rows = 6, 1 + 1                                      # label + row 0 (the reconstruction, then imagination 0)
    assert ego['0']['samples'] == 2 and ego['0']['pairs'] == 2 * rows * (s - 1) and 0 < ego['0']['fitness'] <= 1
    assert ego['0']['pairs_at_max_iteration'] <= ego['0']['pairs']
    traj = [f for f in out['files'] if os.path.basename(os.path.dirname(f)).endswith('_traj')]
    assert [os.path.relpath(f, b) for f in traj] == ['panels/pred0_outputs_0_traj/step00000000_b0.png']       # batch size 1, one batch drawn
    image = png_read(open(traj[0], 'rb').read())
    n_rows = max(cfg.PREDICTION.N_SAMPLES, 1)
    assert image.shape == (196, 196 * (1 + n_rows), 3) and tuple(image[0, 0]) == (50, 50, 50) and (image[..., 0] == 150).any()
    assert not os.path.exists(os.path.join(a, 'ego_motion.json')) and not os.path.exists(os.path.join(a, 'panels'))
    # the path `train --panel-dir DIR --traj` takes: visualise with output_imagines = [] and a label as long as the output
    from muvo_amd.visualise import PanelWriter
    writer = PanelWriter(os.path.join(b, 'train_panels'))
    module.traj_panels, module.traj_options = True, knobs
    try:
        rf = seen['output']['lidar_reconstruction_1'].shape[1]
        batch_rf = {k: v[:, :rf] for k, v in seen['batch'].items() if torch.is_tensor(v)}
        module.visualise(batch_rf, seen['output'], [], 0, prefix='train', writer=writer)
    finally:
        module.traj_panels, module.traj_options = False, {}
    mine = [f for f in writer.files if os.path.basename(os.path.dirname(f)) == 'train_outputs_traj']
    assert len(mine) == 1 and png_read(open(mine[0], 'rb').read()).shape == (196, 392, 3)
