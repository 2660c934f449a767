"""-m gpu: the optical-flow kernels (csrc/flow.hip) against the float64 restatement (tests/flow_reference.py), their batching
and determinism, guards around every buffer they write, argument validation, the colour coding, the `_flow` panel through
`WorldModelTrainer.visualise` and the flow metric.  The bars come from the tables of flow_reference.py (measured on the CPU
with the restatement alone), never from the kernels' output."""
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import flow_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 171


def _frames(dev, *greys):
    return torch.from_numpy(np.stack([R.frames_rgb(g) for g in greys])).to(dev)


@pytest.mark.parametrize('size', R.GPU_SIZES)
def test_flow_against_the_float64_restatement(dev, size):
    from muvo_amd import ops
    cases = R.gpu_cases(*size)
    frames = _frames(dev, *[g for _, a, b in cases for g in (a, b)])
    n = len(cases)
    flow = ops.optical_flow(frames, frames, [2 * i for i in range(n)], [2 * i + 1 for i in range(n)]).cpu().numpy()
    assert flow.shape == (n, 2, *size) and np.isfinite(flow).all()
    bad = []
    for i, (name, _, _) in enumerate(cases):
        d, mask, d32 = R.reference_flow(*size, name)
        assert mask.mean() <= R.MAX_BRANCH_FRAGILE and R.flow_accepted(d32, d, mask, *size)          # the conditions, again
        free, fragile = R.flow_deviation(flow[i], d, mask)
        f32 = float(np.abs(flow[i].astype(np.float64) - d32).max())
        print(f'{size} {name}: {free:.3e} px outside the mask (bar {R.kernel_bar(*size):.3e}), {fragile:.3e} inside (bar {R.FRAGILE_BAR}); '
              f'against the float32 restatement {f32:.3e}')
        if not R.flow_accepted(flow[i], d, mask, *size):
            bad.append((name, free, fragile))
    assert not bad, bad


def _pairs_input(dev, h=45, w=61):
    cases = R.gpu_cases(h, w)
    other = R.shift_pair(h, w, (0.6, 0.9), seed=3)
    greys = [g for _, a, b in cases for g in (a, b)] + list(other)
    return _frames(dev, *greys), [-1, 2, 4, 8, 4], [1, 3, 5, 9, 5]


def test_batched_pairs_equal_their_solo_runs_bit_for_bit(dev):
    from muvo_amd import ops
    frames, pa, pb = _pairs_input(dev)
    both = ops.optical_flow(frames, frames, pa, pb)
    again = ops.optical_flow(frames, frames, pa, pb)
    assert torch.equal(both, again), 'two runs of one call differ'
    assert torch.equal(both[2], both[4]), 'a repeated pair differs from itself'
    assert both[0].abs().max() > 0, 'a white first frame against a texture moves'
    for p in range(len(pa)):
        solo = ops.optical_flow(frames, frames, pa[p:p + 1], pb[p:p + 1])
        assert torch.equal(solo[0], both[p]), f'pair {p} depends on the other pairs of the call'
    # the chunked path (a cap that holds two pairs) is the same again
    was = ops.FLOW_WORKSPACE_CAP
    ops.FLOW_WORKSPACE_CAP = 2 * int(ops.lib().muvo_flow_workspace_bytes(C.c_int64(1), 45, 61))
    try:
        assert torch.equal(ops.optical_flow(frames, frames, pa, pb), both)
    finally:
        ops.FLOW_WORKSPACE_CAP = was


def test_identical_and_white_frames_give_exactly_zero(dev):
    from muvo_amd import ops
    frames, _, _ = _pairs_input(dev)
    flow = ops.optical_flow(frames, frames, [0, -1, 3], [0, -1, 3])
    assert not flow.any()


def _guarded(dev, nbytes, dtype, guard=256):
    buf = torch.full((nbytes + 2 * guard,), SENTINEL, dtype=torch.uint8, device=dev)
    return buf, buf[guard:guard + nbytes].view(dtype), guard


def _intact(buf, guard):
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[-guard:] == SENTINEL).all())


def test_guards_around_output_workspace_and_panel(dev):
    from muvo_amd import ops
    L = ops.lib()
    h, w = 70, 93                                                   # two levels, no multiple of either tile
    cases = R.gpu_cases(h, w)[:2]
    frames = _frames(dev, *[g for _, a, b in cases for g in (a, b)])
    P = 2
    need = int(L.muvo_flow_workspace_bytes(C.c_int64(P), h, w))
    wbuf, ws, g = _guarded(dev, need, torch.float32)
    obuf, out, _ = _guarded(dev, P * 2 * h * w * 4, torch.float32)
    ia, ib = (C.c_int32 * P)(0, 2), (C.c_int32 * P)(1, 3)
    rc = L.muvo_flow_farneback(ops._f(frames), C.c_int64(4), ops._f(frames), C.c_int64(4), h, w, ia, ib, C.c_int64(P), ops._p(ws), C.c_int64(need),
                               ops._p(out), ops._st())
    assert rc == 0, L.muvo_last_error()
    torch.cuda.synchronize()
    assert _intact(wbuf, g) and _intact(obuf, g), 'a guard byte next to the workspace or the flow changed'
    flow = out.view(P, 2, h, w)
    assert torch.equal(flow, ops.optical_flow(frames, frames, [0, 2], [1, 3]))
    # the tile writer: a panel between guards, tiles at an even origin that is no multiple of 4, a sentinel background
    th, tw = h + 10, w + 10                                         # 103 columns: one sentinel column between the tiles keeps the origins even
    pbuf, panel, _ = _guarded(dev, 1 * 3 * (th + 3) * (2 + 2 * (tw + 1)), torch.uint8, guard=66)
    panel = panel.view(1, 3, th + 3, 2 + 2 * (tw + 1))
    ops.flow_colour(flow.contiguous(), panel, ops.tile_place(panel, 2, x0=2, y0=3, xstep=tw + 1))
    torch.cuda.synchronize()
    assert _intact(pbuf, 66)
    host = panel.cpu().numpy()[0]
    assert (host[:, :3] == SENTINEL).all() and (host[:, :, :2] == SENTINEL).all() and (host[:, :, -1] == SENTINEL).all()
    assert (host[:, :, 2 + tw] == SENTINEL).all()
    for k in range(2):
        t = host[:, 3:, 2 + k * (tw + 1):2 + k * (tw + 1) + tw]
        assert (t[:, :5] == 204).all() and (t[:, -5:] == 204).all() and (t[:, :, :5] == 204).all() and (t[:, :, -5:] == 204).all()
        ok, flagged, differ = R.colour_accepted(t[:, 5:-5, 5:-5], flow[k].cpu().numpy())
        assert ok, (k, flagged, differ)


def test_invalid_arguments_return_the_error_code(dev):
    from muvo_amd import ops
    L = ops.lib()
    h, w = 16, 20
    frames = torch.rand(3, 3, h, w, device=dev)
    need = int(L.muvo_flow_workspace_bytes(C.c_int64(1), h, w))
    assert need > 0 and L.muvo_flow_workspace_bytes(C.c_int64(1), 15, w) == -1 and L.muvo_flow_workspace_bytes(C.c_int64(1), h, 15) == -1
    ws = torch.full((need // 4,), 7.0, device=dev)
    out = torch.full((1, 2, h, w), 7.0, device=dev)

    def call(hh, ww, a, b, nbytes):
        return L.muvo_flow_farneback(ops._f(frames), C.c_int64(3), ops._f(frames), C.c_int64(3), hh, ww, (C.c_int32 * 1)(a), (C.c_int32 * 1)(b),
                                     C.c_int64(1), ops._p(ws), C.c_int64(nbytes), ops._p(out), ops._st())
    for args, word in (((15, w, 0, 1, need), b'16..8192'), ((h, w, 3, 1, need), b'outside its stacks'), ((h, w, 0, -2, need), b'outside its stacks'),
                       ((h, w, 0, 1, need - 4), b'workspace')):
        assert call(*args) == -1 and word in L.muvo_last_error(), (args, L.muvo_last_error())
    torch.cuda.synchronize()
    assert bool((ws == 7.0).all()) and bool((out == 7.0).all()), 'a refused call launched something'
    assert call(h, w, 0, 1, need) == 0
    with pytest.raises(ValueError):
        ops.optical_flow(frames[:, :, :15], frames[:, :, :15], [0], [1])
    with pytest.raises(RuntimeError, match='outside its stacks'):
        ops.optical_flow(frames, frames, [0], [3])
    # the tile writer: an odd tile origin, a panel narrower than the tile
    flow = torch.zeros(1, 2, h, w, device=dev)
    panel = torch.full((1, 3, h + 10, w + 12), SENTINEL, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match='odd column'):
        ops.flow_colour(flow, panel, ops.tile_place(panel, 1, x0=1))
    narrow = torch.full((1, 3, h + 10, w + 8), SENTINEL, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match='leaves the'):
        ops.flow_colour(flow, narrow, ops.tile_place(narrow, 1))
    assert bool((panel == SENTINEL).all()) and bool((narrow == SENTINEL).all())
    ops.flow_colour(flow, panel, ops.tile_place(panel, 1, x0=2))
    host = panel.cpu().numpy()[0]
    assert (host[:, 5:-5, 7:-5] == 255).all() and (host[:, :, 2:7] == 204).all() and (host[:, :, :2] == SENTINEL).all()   # zero flow: all 255


@pytest.mark.parametrize('size', [(45, 61), (131, 150)])
def test_colour_kernel_against_the_restatement(dev, size):
    from muvo_amd import ops
    h, w = size
    fields = np.stack([R.zoom_field(h, w), R.rotation_field(h, w)])
    flow = torch.from_numpy(fields).to(dev)
    panel = torch.zeros((2, 3, h + 10, w + 10), dtype=torch.uint8, device=dev)
    ops.flow_colour(flow, panel, ops.tile_place(panel, 1))
    host = panel.cpu().numpy()
    for k in range(2):
        want = R.tile(fields[k])
        assert (host[k][:, :5] == 204).all() and (want[:, :5] == 204).all()
        ok, flagged, differ = R.colour_accepted(host[k][:, 5:-5, 5:-5], fields[k])
        print(f'{size} field {k}: {flagged:.4f} quantisation-fragile, {differ} bytes differ from the float64 coding')
        assert flagged <= R.MAX_QUANT_FRAGILE and ok
        assert len(np.unique(host[k][:, 5:-5, 5:-5])) > 50


# ---- the panel and the metric ----------------------------------------------------------------------------------------------------
H, W, B, S, RF = 48, 64, 2, 4, 2


def _sequence(seed, n, zoom, shift, t0=0):
    """n frames (n, 3, H, W) float32 of one texture under a growing zoom about an off-centre point plus a drift"""
    f = R.texture_fn(seed)
    out = []
    for t in range(t0, t0 + n):
        z, cx, cy = zoom ** t, 0.4 * W, 0.55 * H
        out.append(R.frames_rgb(R.frame_bytes(f, H, W, lambda x, y: (cx + (x - cx) / z - shift[0] * t, cy + (y - cy) / z - shift[1] * t))))
    return np.stack(out)


@pytest.fixture(scope='module')
def scene():
    label = np.stack([_sequence(10 + n, S, 1.05, (0.4, -0.3)) for n in range(B)])
    recon = np.stack([_sequence(10 + n, RF, 1.06, (0.2, 0.1)) for n in range(B)])
    imagines = [np.stack([_sequence(10 + n, S - RF, 1.04 + 0.02 * i, (0.5, 0.2 * i), t0=RF) for n in range(B)]) for i in range(2)]
    return label, recon, imagines


def _dicts(dev, label, recon, imagines):
    batch = {'rgb_label_1': torch.from_numpy(label).to(dev), 'throttle_brake': torch.zeros(B, S, 1, device=dev), 'steering': torch.zeros(B, S, 1, device=dev)}
    return batch, {'rgb_1': torch.from_numpy(recon).to(dev)}, [{'rgb_1': torch.from_numpy(im).to(dev)} for im in imagines]


class _Writer:
    def __init__(self):
        self.images = {}

    def add_images(self, name, tensor, global_step=0):
        self.images[name] = tensor.cpu().numpy()

    def add_video(self, name, tensor, global_step=0, fps=2):
        self.images[name] = tensor.cpu().numpy()


def _visualise(cfg, flow_panels, batch, output, imagines):
    from muvo_amd.trainer import WorldModelTrainer
    stub = types.SimpleNamespace(cfg=cfg, panel_writer=None, traj_panels=False, traj_options={}, flow_panels=flow_panels, _step_now=lambda: 0)
    writer = _Writer()
    WorldModelTrainer.visualise(stub, batch, output, imagines, 0, prefix='val', writer=writer)
    return writer.images


def test_visualise_without_the_switch_is_unchanged(dev, scene):
    """flow_panels = False: the names and bytes written are those of render_panels alone (holds before the flow existed too)"""
    import visualise_reference as VR
    from muvo_amd.visualise import render_panels
    cfg = VR.panel_cfg(rgb=True)
    batch, output, ims = _dicts(dev, *scene)
    off = _visualise(cfg, False, batch, output, ims)
    want = render_panels(cfg, batch, output, ims)
    assert list(off) == [f'val_outputs_0{k}' for k in want] == ['val_outputs_0_rgb']
    assert all(np.array_equal(off[f'val_outputs_0{k}'], v.cpu().numpy()) for k, v in want.items())


def test_flow_panel_through_visualise(dev, scene):
    import visualise_reference as VR
    cfg = VR.panel_cfg(rgb=True)
    label, recon, imagines = scene
    batch, output, ims = _dicts(dev, label, recon, imagines)
    off = _visualise(cfg, False, batch, output, ims)
    on = _visualise(cfg, True, batch, output, ims)
    assert list(off) == ['val_outputs_0_rgb'] and list(on) == ['val_outputs_0_rgb', 'val_outputs_0_flow']
    assert np.array_equal(off['val_outputs_0_rgb'], on['val_outputs_0_rgb'])
    got = on['val_outputs_0_flow']
    th, tw = H + 10, W + 10
    assert got.shape == (B, 3, 3 * th, (S - 1) * tw) and got.dtype == np.uint8
    white = np.ones((B, RF, 3, H, W), np.float32)
    rows = [np.concatenate([recon if i == 0 else white, imagines[i]], axis=1) for i in range(2)]
    checked = [0, 0.0]

    def tile_fn(a, b):
        g0, g1 = R.grey_of(a), R.grey_of(b)
        d, mask = R.farneback(g0, g1, np.float64, with_mask=True)
        tol = max(8.0 * float(np.abs(R.farneback(g0, g1, np.float32) - d).max()), 1e-4)
        tile_fn.flows.append((d, tol, mask))
        return R.tile(d)
    tile_fn.flows = []
    want = R.panel(label, rows, RF, tile_fn)
    at = 0
    for bs in range(B):                                   # the order R.panel asks for its tiles
        for step in range(1, S):
            for r in range(3):
                d, tol, mask = tile_fn.flows[at]
                at += 1
                mine = got[bs, :, r * th:(r + 1) * th, (step - 1) * tw:step * tw]
                ref = want[bs, :, r * th:(r + 1) * th, (step - 1) * tw:step * tw]
                assert (mine[:, :5] == 204).all() and (mine[:, -5:] == 204).all() and (mine[:, :, :5] == 204).all() and (mine[:, :, -5:] == 204).all()
                if not d.any():
                    assert (mine[:, 5:-5, 5:-5] == 255).all() and (ref[:, 5:-5, 5:-5] == 255).all()
                    continue
                ok, flagged, differ = R.colour_accepted(mine[:, 5:-5, 5:-5], d, flow_tol=tol, skip=mask)
                checked[0] += 1
                checked[1] = max(checked[1], flagged)
                assert ok, (bs, step, r, flagged, differ, tol)
                assert differ <= 0.05 * mine[:, 5:-5, 5:-5].size, (bs, step, r, differ)
    print(f'{checked[0]} flow tiles compared, at most {checked[1]:.3f} of a tile quantisation-fragile under its flow tolerance')
    assert at == len(tile_fn.flows) and checked[0] == B * (S - 1) * 3 - B * 1      # rows i > 0: one white-white tile per sample
    # without imagined samples the row ends after the reconstructed steps
    short = _visualise(VR.panel_cfg(), True, batch, output, [])
    assert short == {}                                    # no camera head, no panel
    from muvo_amd.flow import flow_panel
    short = flow_panel(batch, output, []).cpu().numpy()
    assert short.shape == (B, 3, 2 * th, (S - 1) * tw) and (short[:, :, th:, (RF - 1) * tw:] == 255).all()
    assert np.array_equal(short[:, :, :th], got[:, :, :th]) and np.array_equal(short[:, :, th:, :tw], got[:, :, th:2 * th, :tw])


def test_flow_metric(dev, tmp_path):
    from muvo_amd.flow import FlowMetric
    # the prediction IS the record: 0; the prediction drifts by a known extra amount per step: that amount
    extra = (0.8, -0.6)
    label = np.stack([_sequence(10 + n, S, 1.0, (0.4, -0.3)) for n in range(B)])
    moved = np.stack([_sequence(10 + n, S, 1.0, (0.4 + extra[0], -0.3 + extra[1])) for n in range(B)])
    for pred, want in ((label, 0.0), (moved, float(np.hypot(*extra)))):
        batch, output, ims = _dicts(dev, label, pred[:, :RF], [pred[:, RF:]])
        m = FlowMetric()
        m.start_loader(1)
        m.update(0, batch, output, ims)
        m.update(1, batch, output, ims)
        res = m.result()
        assert set(res) == {f'test1_flow_{k}' for k in ('epe', 'epe_imagine', 'magnitude', 'magnitude_imagine', 'pairs', 'pairs_imagine')}
        print(res)
        assert res['test1_flow_pairs'] == 2 * B * (RF - 1) and res['test1_flow_pairs_imagine'] == 2 * B * (S - RF - 1)
        for key in ('test1_flow_epe', 'test1_flow_epe_imagine'):
            assert abs(res[key] - want) <= (0.0 if want == 0.0 else R.recovery_bar(45, 61)), (key, res[key], want)
        assert res['test1_flow_magnitude'] > 0.3
    path = m.write(str(tmp_path))
    assert os.path.basename(path) == 'optical_flow.json' and json.load(open(path)) == res


def test_predict_optical_flow_leaves_the_metrics_alone(dev, tmp_path):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd import ops
    from muvo_amd import predict as P
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    root = str(tmp_path / 'rec')
    os.makedirs(root)
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1, STEPS=100000)
    torch.manual_seed(79)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    assert module.flow_panels is False and cfg.EVAL.RGB_SUPERVISION

    def data():
        dm = DataModule(cfg, root, device=dev, seed=79)
        dm.setup()
        dm.test_sampler_0 = range(0, 4, 2)
        return dm
    a, b = str(tmp_path / 'plain'), str(tmp_path / 'flow')
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        P.run(cfg, dev, a, 'test', loaders=[0], limit_batches=2, seed=79, data=data(), module=module, log=lambda s: None)
        out = P.run(cfg, dev, b, 'test', loaders=[0], limit_batches=2, seed=79, data=data(), module=module, log=lambda s: None, panels=1,
                    flow=True, optical_flow=True)
    finally:
        ops.set_deterministic(was)
    assert open(os.path.join(a, 'metrics.json'), 'rb').read() == open(os.path.join(b, 'metrics.json'), 'rb').read()
    assert module.flow_panels is False and module.panel_writer is None
    res = json.load(open(os.path.join(b, 'optical_flow.json')))
    assert res == out['optical_flow'] and set(res) == {f'test0_flow_{k}' for k in ('epe', 'epe_imagine', 'magnitude', 'magnitude_imagine', 'pairs', 'pairs_imagine')}
    assert all(np.isfinite(v) and v >= 0 for v in res.values()) and res['test0_flow_pairs'] == 2 * 1 and res['test0_flow_pairs_imagine'] == 2 * 3
    flows = [f for f in out['files'] if os.path.basename(os.path.dirname(f)).endswith('_flow')]
    assert [os.path.relpath(f, b) for f in flows] == ['panels/pred0_outputs_0_flow/step00000000_b0.png']
    assert not os.path.exists(os.path.join(a, 'optical_flow.json')) and not os.path.exists(os.path.join(a, 'panels'))
    from muvo_amd.visualise import png_read
    image = png_read(open(flows[0], 'rb').read())
    n_rows = max(cfg.PREDICTION.N_SAMPLES, 1)                 # s = 6: five columns
    assert image.shape[2] == 3 and image.shape[0] % (1 + n_rows) == 0 and image.shape[1] % 5 == 0 and tuple(image[0, 0]) == (204, 204, 204)
