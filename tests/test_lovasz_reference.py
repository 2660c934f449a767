"""CPU: the float64 restatement of the Lovasz-softmax loss (tests/lovasz_reference.py) against a brute-force evaluation of the
definition and against plain autograd, its closed forms against the difference form, the bars against planted errors, and the
configuration surface of the extension key LOSSES.VOXEL_LOVASZ."""
import argparse
import itertools
import types

import pytest
import torch

import lovasz_reference as R
import loss_reference as LR


# ------------------------------------------------------------------------------------------------ restatement vs the definition
def _brute(logits, labels):
    """loss (weight 1) and dlde of the definition, rank by rank from explicit index sets: J(S) = 1 - |fg \\ S| / |fg u S| for the
    set S of the voxels ranked so far, g_i = J(S_i) - J(S_{i-1}) in exact rational arithmetic"""
    from fractions import Fraction
    F, C, V = logits.shape
    p = torch.softmax(logits.double(), 1)
    total = 0.0
    dlde = torch.zeros(F, C, V, dtype=torch.float64)
    for f in range(F):
        valid = [v for v in range(V) if int(labels[f, v]) < C]
        frame, npres = 0.0, 0
        for c in range(C):
            fg = {v for v in valid if int(labels[f, v]) == c}
            if not fg:
                continue
            npres += 1
            e = {v: float(1 - p[f, c, v]) if v in fg else float(p[f, c, v]) for v in valid}
            ranked = sorted(valid, key=lambda v: (-e[v], v))
            S, J_prev = set(), Fraction(0)
            for v in ranked:
                S.add(v)
                J = 1 - Fraction(len(fg - S), len(fg | S))
                g = J - J_prev
                J_prev = J
                dlde[f, c, v] = float(g)
                frame += e[v] * float(g)
        total += frame / max(1, npres)
    return total / F, dlde


def _small_inputs():
    """n <= 12 voxels, C = 2 and 3, logits from a few levels (every tie pattern of n <= 4 exhaustively for C = 2, random draws
    above), labels with ignored voxels and absent classes among them"""
    out = []
    for n in (1, 2, 3, 4):
        for lab in itertools.product((0, 1, 255), repeat=n):
            for lev in itertools.product((0.0, 1.0), repeat=n):
                out.append((torch.tensor([[lev, [0.0] * n]]), torch.tensor([lab], dtype=torch.uint8)))
    g = torch.Generator().manual_seed(5)
    for k in range(150):
        n, C, F = int(torch.randint(5, 13, (1,), generator=g)), 2 + k % 2, 1 + k % 3
        logits = torch.randint(0, 3, (F, C, n), generator=g).float() if k % 2 else torch.randn(F, C, n, generator=g)
        labels = torch.randint(0, C + 1, (F, n), generator=g).to(torch.uint8)
        labels[labels == C] = 255 if k % 4 else C
        out.append((logits, labels))
    return out


def test_restatement_matches_the_definition_rank_by_rank():
    worst = 0.0
    for logits, labels in _small_inputs():
        loss, dlde = _brute(logits, labels)
        ref = R.lovasz64(logits, labels)
        assert abs(float(ref['loss']) - loss) <= 1e-12, (logits, labels)
        worst = max(worst, float((ref['dlde'] - dlde).abs().max()))
        assert float(ref['loss']) <= 1.0 + 1e-12
    print(f'LOSSSTAT brute-force dlde: {worst:.3e}')
    assert worst <= 1e-12


@pytest.mark.parametrize('shape', [(2, 2, 4099), (2, 9, 4099), (1, 3, 70001)], ids=str)
def test_closed_forms_equal_the_difference_form(shape):
    F, C, V = shape
    g = torch.Generator().manual_seed(V + C)
    fgs = torch.rand(V, generator=g) < 0.1
    closed = R.jaccard_increments(fgs)
    G, cum = int(fgs.sum()), torch.cumsum(fgs.long(), 0)
    i = torch.arange(1, V + 1)
    J = 1 - (G - cum).double() / (G + (i - cum)).double()
    diff = J - torch.cat([torch.zeros(1, dtype=torch.float64), J[:-1]])
    assert float((closed - diff).abs().max()) <= 1e-12
    assert abs(float(closed.sum()) - 1.0) <= 1e-12           # the increments add up to J_n = 1
    assert not R.jaccard_increments(torch.zeros(V, dtype=torch.bool)).any()


def _autograd(logits, labels, weight):
    """the loss through torch.sort + cumsum in float64, differentiated by autograd (Berman's lovasz_grad, per frame, 'present')"""
    F, C, V = logits.shape
    z = logits.double().requires_grad_(True)
    p = torch.softmax(z, 1)
    total = 0
    for f in range(F):
        vox = (labels[f].long() < C).nonzero()[:, 0]
        terms = []
        for c in range(C):
            fg = (labels[f, vox].long() == c).double()
            if not fg.any():
                continue
            e = (fg - p[f, c, vox]).abs()
            es, perm = torch.sort(e, descending=True)
            fs = fg[perm]
            inter = fs.sum() - fs.cumsum(0)
            union = fs.sum() + (1 - fs).cumsum(0)
            J = 1 - inter / union
            J = torch.cat([J[:1], J[1:] - J[:-1]])
            terms.append((es * J).sum())
        if terms:
            total = total + sum(terms) / len(terms)
    loss = weight * total / F
    grad, = torch.autograd.grad(loss, z)
    return loss.detach(), grad


@pytest.mark.parametrize('id', ['F2-C2-V4099-mix', 'F2-C9-V4099-mix', 'F2-C2-V257-frame-all-ignored'])
def test_restatement_matches_autograd_without_ties(id):
    logits, labels = R.inputs(id)
    ref = R.reference(id)
    e = ref['errors']
    for f in range(e.shape[0]):                               # random logits: no two valid voxels of a segment tie
        for c in range(e.shape[1]):
            v = e[f, c][labels[f].long() < e.shape[1]]
            assert v.unique().numel() == v.numel()
    loss, grad = _autograd(logits, labels, R.WEIGHT)
    assert abs(float(loss) - float(ref['loss'])) <= 1e-12 * max(1.0, abs(float(loss)))
    st = LR.error_stats(ref['dlogits'], grad, LR.scale_of(grad))
    print(f'LOSSSTAT {id} restatement-vs-autograd dlogits: {st["max_e"]:.3e}')
    assert st['max_e'] <= 1e-12


def test_value_properties():
    g = torch.Generator().manual_seed(11)
    F, C, V = 2, 3, 500
    labels = R.mix_labels(F, C, V, g)
    onehot = torch.full((F, C, V), -30.0)
    for c in range(C):
        onehot[:, c][labels == c] = 30.0
    assert 0 <= float(R.lovasz64(onehot, labels)['loss']) < 1e-9
    logits = 2 * torch.randn(F, C, V, generator=g)
    for w in (1.0, R.WEIGHT):
        assert float(R.lovasz64(logits, labels, w)['loss']) <= w
        assert float(R.lovasz64(-onehot, labels, w)['loss']) <= w * (1 + 1e-12)       # everything wrong: the largest value
    ref = R.lovasz64(logits, labels, R.WEIGHT)
    garbage = logits.clone()
    ign = (labels.long() >= C)[:, None, :].expand(F, C, V)
    garbage[ign] = 1e4 * torch.randn(int(ign.sum()), generator=g)
    other = R.lovasz64(garbage, labels, R.WEIGHT)
    assert torch.equal(other['loss'], ref['loss']) and torch.equal(other['dlogits'], ref['dlogits'])
    assert not ref['dlogits'][ign].any() and not ref['dlde'][ign].any()
    # a frame without a valid voxel contributes 0 and still counts in F
    two = R.lovasz64(torch.cat([logits[:1], logits[:1]]), torch.stack([labels[0], torch.full((V,), 255, dtype=torch.uint8)]))
    one = R.lovasz64(logits[:1], labels[:1])
    assert abs(float(two['loss']) - float(one['loss']) / 2) <= 1e-15
    assert not two['present'][1].any() and not two['dlogits'][1].any()


# ------------------------------------------------------------------------------------------------ bars vs planted errors
def _bad(got, ref, names=('loss', 'dlogits', 'errors', 'dlde')):
    return set(R.failures(R.compare(got, ref, names)))


@pytest.mark.parametrize('id', [c['id'] for c in R.CASES if c['content'] != 'scale1'])
def test_float32_evaluation_is_within_the_bars(id):
    logits, labels = R.inputs(id)
    ref = R.reference(id)
    mine = R.lovasz64(logits, labels, R.WEIGHT, R.GOUT, dtype=torch.float32)
    handed = R.lovasz64(logits, labels, R.WEIGHT, R.GOUT, dtype=torch.float32, order_from=ref['errors'])
    cmp = {**R.compare(mine, ref, ('loss', 'errors')), **R.compare(handed, ref, ('dlde', 'dlogits'))}
    for line in R.statlines(id + ' float32', cmp):
        print(line)
    assert not R.failures(cmp)


@pytest.mark.parametrize('id', ['F2-C2-V4099-mix', 'F2-C9-V4099-mix', 'F1-C3-V16384-quantised-tie-runs'])
def test_bars_reject_planted_errors(id):
    logits, labels = R.inputs(id)
    ref = R.reference(id)
    F, C, V = logits.shape
    # two adjacent ranks of different kind swapped in dlde
    f, c = F - 1, 0
    vox = (labels[f].long() < C).nonzero()[:, 0]
    ranked = vox[torch.sort(-ref['errors'][f, c, vox], stable=True).indices]
    kinds = labels[f, ranked].long() == c
    i = int((kinds[1:] != kinds[:-1]).nonzero()[len(ranked) // 8 if id.startswith('F2-C2') else 0, 0])
    a, b = int(ranked[i]), int(ranked[i + 1])
    got = {'dlde': ref['dlde'].clone()}
    got['dlde'][f, c, a], got['dlde'][f, c, b] = ref['dlde'][f, c, b], ref['dlde'][f, c, a]
    assert _bad(got, ref) == {'dlde'}
    # one ignored voxel counted as background
    v = int((labels[0].long() >= C).nonzero()[0, 0])
    got = R.lovasz64(logits, labels, R.WEIGHT, R.GOUT, count_ignored=(0, v))
    assert 'dlde' in _bad(got, ref, ('loss', 'dlde', 'dlogits'))
    # 1 / #classes instead of 1 / #present (class C - 1 is absent from frame 0)
    assert not ref['present'][0, C - 1] and ref['present'][0, :C - 1].all()
    got = R.lovasz64(logits, labels, R.WEIGHT, R.GOUT, mean_over_all_classes=True)
    assert _bad(got, ref) == {'loss', 'dlogits'}
    # a tie broken by descending index
    if 'tie-runs' in id:
        got = R.lovasz64(logits, labels, R.WEIGHT, R.GOUT, descending_ties=True)
        assert abs(float(got['loss']) - float(ref['loss'])) <= 1e-12           # the value cannot tell; dlde does
        assert {'dlde', 'dlogits'} <= _bad(got, ref)


def test_constant_logits_rank_by_voxel_index():
    id = 'F1-C4-V8192-constant-logits'
    logits, labels = R.inputs(id)
    ref = R.reference(id)
    C = logits.shape[1]
    valid = labels[0].long() < C
    for c in (0, 1):
        assert bool((ref['errors'][0, c][valid] == 0.5).all())
        assert torch.equal(ref['dlde'][0, c], R.index_order_dlde(labels, C, 0, c))
    got = R.lovasz64(logits, labels, R.WEIGHT, R.GOUT, descending_ties=True)
    assert 'dlde' in _bad(got, ref)


def test_all_foreground_known_answer():
    id = 'F1-C2-V8192-all-foreground'
    logits, labels = R.inputs(id)
    ref = R.reference(id)
    valid = labels[0] == 1
    G = int(valid.sum())
    assert ref['present'].tolist() == [[False, True]]
    assert torch.equal(ref['dlde'][0, 1][valid], torch.full((G,), 1.0 / G, dtype=torch.float64)) and not ref['dlde'][0, 0].any()
    assert not ref['dlde'][0, 1][~valid].any()


# ------------------------------------------------------------------------------------------------ configuration
def test_defaults_do_not_carry_the_key():
    from muvo_amd import config
    cfg = config.get_cfg()
    assert 'VOXEL_LOVASZ' not in cfg.LOSSES and 'VOXEL_LOVASZ' not in config.base_1d_cfg().LOSSES
    assert config.voxel_lovasz(cfg) == (0.0, (1, 2, 4))
    import glob
    import yaml
    for path in glob.glob(config.os.path.join(config._HERE, 'configs', '*.yml')):
        assert 'VOXEL_LOVASZ' not in open(path).read(), path
    assert 'VOXEL_LOVASZ' not in yaml.safe_dump(config.base_1d_cfg().convert_to_dict())


def test_key_round_trips_through_yaml_dict_and_override(tmp_path):
    from muvo_amd import config
    y = tmp_path / 'lv.yml'
    y.write_text('VOXEL_SEG: {ENABLED: true}\nLOSSES:\n  VOXEL_LOVASZ: {WEIGHT: 0.5, FACTORS: [2, 4]}\n')
    cfg = config.get_cfg(argparse.Namespace(config_file=str(y), opts=[]))
    assert config.voxel_lovasz(cfg) == (0.5, (2, 4))
    assert cfg.convert_to_dict()['LOSSES']['VOXEL_LOVASZ'] == {'WEIGHT': 0.5, 'FACTORS': [2, 4]}
    again = config.get_cfg(cfg_dict=cfg.convert_to_dict())                   # the dict a checkpoint carries
    assert config.voxel_lovasz(again) == (0.5, (2, 4))
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_LOVASZ': {'WEIGHT': 2}}})
    assert config.voxel_lovasz(cfg) == (2.0, (1, 2, 4))                       # FACTORS absent: [1, 2, 4]
    cfg = config.get_cfg(argparse.Namespace(config_file='', opts=['VOXEL_SEG.ENABLED', 'True', 'LOSSES.VOXEL_LOVASZ.WEIGHT', '0.25',
                                                                  'LOSSES.VOXEL_LOVASZ.FACTORS', '[4]']))
    assert config.voxel_lovasz(cfg) == (0.25, (4,))
    cfg = config.base_1d_cfg(**{'LOSSES.VOXEL_LOVASZ.WEIGHT': 0.5})
    assert config.voxel_lovasz(cfg) == (0.5, (1, 2, 4))
    with pytest.raises(KeyError):
        config.get_cfg().merge_from_list(['LOSSES.VOXEL_LOVAS.WEIGHT', '1'])


@pytest.mark.parametrize('factors', [[3], [2, 8], [0], [2, 2], 2, [True]], ids=str)
def test_bad_factors_raise(factors):
    from muvo_amd import config
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_LOVASZ': {'WEIGHT': 1.0, 'FACTORS': factors}}})
    with pytest.raises(ValueError, match='FACTORS'):
        config.voxel_lovasz(cfg)


def test_bad_weight_and_disabled_head_raise():
    from muvo_amd import config
    with pytest.raises(ValueError, match='VOXEL_SEG.ENABLED'):
        config.voxel_lovasz(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False}, 'LOSSES': {'VOXEL_LOVASZ': {'WEIGHT': 1.0}}}))
    assert config.voxel_lovasz(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False}, 'LOSSES': {'VOXEL_LOVASZ': {'WEIGHT': 0.0}}}))[0] == 0.0
    for w in (-1.0, 'much', True):
        with pytest.raises(ValueError, match='WEIGHT'):
            config.voxel_lovasz(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_LOVASZ': {'WEIGHT': w}}}))


def test_compute_loss_key_set_with_and_without_the_key(monkeypatch):
    """the trainer's wiring with the kernels stubbed out: without the key today's terms and no Lovasz call; with it one call per
    configured factor, on the head's tensors as they are, with weight WEIGHT / f, after every other term"""
    from muvo_amd import ops
    from muvo_amd.trainer import WorldModelTrainer
    calls = []
    monkeypatch.setattr(ops, 'voxel_losses', lambda logits, target, weight, cw=None, terms=False: tuple(torch.zeros(()) for _ in range(3)))

    def lovasz(logits, labels, weight, terms=False):
        calls.append((logits, labels, weight, terms))
        return (torch.zeros(()),)
    monkeypatch.setattr(ops, 'voxel_lovasz_loss', lovasz)
    batch, output = R.voxel_dicts()
    today = [f'{name}_{f}' for f in (1, 2, 4) for name in ('voxel', 'sem_scal', 'geo_scal')]
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=R.voxel_only_cfg()), batch, output)
    assert list(losses) == today and not calls
    cfg = R.voxel_only_cfg(**{'LOSSES.VOXEL_LOVASZ.WEIGHT': 0.5})
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)
    assert list(losses) == today + ['voxel_lovasz_1', 'voxel_lovasz_2', 'voxel_lovasz_4']
    assert [(c[2], c[3]) for c in calls] == [(0.5, True), (0.25, True), (0.125, True)]
    for k, f in enumerate((1, 2, 4)):
        assert calls[k][0] is output[f'voxel_{f}'] and calls[k][1] is batch[f'voxel_label_{f}']
    del calls[:]
    cfg = R.voxel_only_cfg(**{'LOSSES.VOXEL_LOVASZ.WEIGHT': 0.5, 'LOSSES.VOXEL_LOVASZ.FACTORS': [2]})
    assert list(WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)) == today + ['voxel_lovasz_2']
    assert calls[0][2] == 0.25 and calls[0][0] is output['voxel_2']
    del calls[:]
    cfg = R.voxel_only_cfg(**{'LOSSES.VOXEL_LOVASZ.WEIGHT': 0.0})
    assert list(WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)) == today and not calls


def test_validation_curves_pick_the_terms_up_by_name():
    """the validation loss curves are keyed by the names compute_loss returns: the pass lists no loss term by hand"""
    import inspect
    from muvo_amd import validate
    src = inspect.getsource(validate)
    assert "{f'val{idx}_{k}': v for k, v in loss.items()}" in src and "for k, v in loss_imagines[0].items()" in src
    assert 'voxel_lovasz' not in src and 'lidar_cd' not in src and 'sem_scal' not in src


def test_module_guards():
    from muvo_amd.losses import LovaszSoftmaxLoss
    crit = LovaszSoftmaxLoss()
    assert crit.ignore_index == 255
    with pytest.raises(ValueError):
        crit(torch.zeros(1, 2, 5, 4), torch.zeros(1, 2, 5, 4))
    with pytest.raises(ValueError, match='ignore_index'):
        LovaszSoftmaxLoss(ignore_index=1)(torch.zeros(1, 1, 2, 2, 2, 2), torch.zeros(1, 1, 1, 2, 2, 2, dtype=torch.uint8))


def test_entry_points_validate_before_touching_the_device():
    """bad arguments come back as MUVO_ERR_INVALID_ARG with a message; nothing is launched (this runs without a GPU)"""
    import ctypes as C
    from muvo_amd import ops
    L = ops.lib()
    p, null = C.c_void_p(256), C.c_void_p(0)      # never dereferenced: every call below is rejected by its argument checks
    i64, st, w = C.c_int64, C.c_void_p(0), C.c_float(1.0)
    assert L.muvo_lovasz_ws_bytes(i64(20), 2, i64(36864)) >= 16 * 20 * 2 * 36864            # keys and payload, twice, for 40 segments
    assert L.muvo_lovasz_ws_bytes(i64(1), 1, i64(8)) == 0 and L.muvo_lovasz_ws_bytes(i64(1), 17, i64(8)) == 0
    # the transient part is bounded: 20 frames x 9 classes at scale 1 need less than twice what 3 frames' ping-pong buffers take
    V1 = 192 * 192 * 64
    assert L.muvo_lovasz_ws_bytes(i64(20), 9, i64(V1)) < 2 * 16 * 3 * 9 * V1
    for C_ in (1, 17):
        assert L.muvo_lovasz_fwd(p, p, i64(2), C_, i64(8), w, p, p, p, p, p, st) == -1
        assert b'classes (2..16)' in L.muvo_last_error()
        assert L.muvo_lovasz_bwd(p, p, p, p, p, i64(2), C_, i64(8), w, p, st) == -1
    assert L.muvo_lovasz_fwd(p, p, i64(32768), 2, i64(8), w, p, p, p, p, p, st) == -1
    assert b'65535' in L.muvo_last_error()
    assert L.muvo_lovasz_fwd(p, p, i64(2), 2, i64((1 << 30) + 1), w, p, p, p, p, p, st) == -1
    assert b'2^30' in L.muvo_last_error()
    assert L.muvo_lovasz_fwd(p, p, i64(2), 2, i64(0), w, p, p, p, p, p, st) == -1
    assert L.muvo_lovasz_fwd(p, null, i64(2), 2, i64(8), w, p, p, p, p, p, st) == -1
    assert b'lovasz_fwd: null pointer' in L.muvo_last_error()
    assert L.muvo_lovasz_fwd(p, p, i64(2), 2, i64(8), w, p, null, null, null, p, st) == -1         # present is not optional
    assert L.muvo_lovasz_bwd(p, p, null, p, p, i64(2), 2, i64(8), w, p, st) == -1
    assert b'lovasz_bwd: null pointer' in L.muvo_last_error()
    assert L.muvo_lovasz_bwd(p, p, p, p, p, i64(32768), 2, i64(8), w, p, st) == -1
