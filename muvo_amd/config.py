"""Config surface of the reference (muvo/config.py:1-369): `get_parser()`, `get_cfg(args, cfg_dict)`,
`CfgNode.convert_to_dict()`, every default key — on an own minimal yacs-style node (fvcore/yacs are not
dependencies).  Differences, on purpose: YAML files may carry the three keys of the reference's unreleased 2-D
branch (TOLERATED_EXTRA_KEYS); they are accepted and dropped instead of raising KeyError."""
import argparse
import copy
import os

import yaml

_HERE = os.path.dirname(os.path.abspath(__file__))
TOLERATED_EXTRA_KEYS = ('CML_DATASET_VERSION', 'MODEL.TRANSFORMER_TRANSITION', 'LOSSES.PERCEPTUAL')
# Extension keys (NOT in the reference, absent from the defaults so that the default config stays equal to the reference's;
# accepted from YAML files, cfg dicts and command-line overrides, and kept):
#   MODEL.CONSTANT_SIZE.{RGB,LIDAR,VOXEL} - the seed sizes the reference hard-codes as (5, 13), (1, 16) and (3, 3, 1)
#   (muvo/models/mile.py:322-336,391-396): every decoder output is 64x its seed, so (1, 32) gives the 64 x 2048 range view and
#   (4, 4, 1) the 256 x 256 x 64 voxel grid BASELINE.json names.  Parity for non-default values: own oracle only ("unpinned").
#   LOSSES.LIDAR_CD.{WEIGHT,FACTORS} - the Chamfer-distance loss of the lidar reconstruction head, which the reference defines
#   (CDLoss, muvo/losses.py:352-367) but only constructs in a comment (muvo/trainer.py:116).  WEIGHT (float; absent = 0 = off)
#   multiplies, FACTORS (a list drawn from 1, 2, 4; absent = [2, 4]) names the output scales that get a term
#   `lidar_cd_{f}` = WEIGHT / f x CD(lidar_reconstruction_f[:, :, :3], range_view_label_f[:, :, :3]).  The search is brute force:
#   factor 1 (65,536 points a frame) is left out of the default list for its cost.  Needs LIDAR_RE.ENABLED.
#   LOSSES.VOXEL_LOVASZ.{WEIGHT,FACTORS} - the Lovasz-softmax loss of the voxel head (the surrogate of the IoU the head is judged
#   by; the reference has none).  WEIGHT (float; absent = 0 = off) multiplies, FACTORS (a list drawn from 1, 2, 4; absent =
#   [1, 2, 4]) names the output scales that get a term `voxel_lovasz_{f}` = WEIGHT / f x Lovasz(voxel_f, voxel_label_f), every
#   frame a segment of its own, classes 'present' (DESIGN.md section 11).  Needs VOXEL_SEG.ENABLED.
#   LOSSES.VOXEL_RENDER.{WEIGHT,FACTORS,STRIDE} - the rendered first-hit depth loss of the voxel head along lidar rays (what the
#   RayIoU metric measures; the reference has none).  WEIGHT (float; absent = 0 = off) multiplies, FACTORS (a list drawn from
#   1, 2, 4; absent = [1, 2, 4]) names the output scales that get a term `voxel_render_{f}` = WEIGHT / f x render(voxel_f,
#   voxel_label_f) x VOXEL.RESOLUTION f / LIDAR_RE.SCALE (the scaled depth units of lidar_depth_f), STRIDE (an integer >= 1;
#   absent = 1) takes every STRIDE-th azimuth of the range view as a ray.  Needs VOXEL_SEG.ENABLED.
#   LOSSES.VOXEL_RENDER_CLASS.{WEIGHT,FACTORS,STRIDE} - the rendered first-hit class loss of the voxel head along the same rays
#   (the class half of RayIoU; the reference has none).  WEIGHT (float; absent = 0 = off) multiplies, FACTORS (a list drawn from
#   1, 2, 4; absent = [1, 2, 4]) names the output scales that get a term `voxel_render_class_{f}` = WEIGHT / f x
#   render_class(voxel_f, voxel_label_f), STRIDE (an integer >= 1; absent = 1) takes every STRIDE-th azimuth of the range view as
#   a ray - the table LOSSES.VOXEL_RENDER uses at the same stride.  Needs VOXEL_SEG.ENABLED.
#   LOSSES.VOXEL_BOUNDARY.{WEIGHT,FACTORS,TRUNCATE_M} - the distance-transform boundary loss of the voxel head (a wrong voxel costs
#   its distance to the other set's surface; the reference has none).  WEIGHT (float; absent = 0 = off) multiplies, FACTORS (a
#   list drawn from 1, 2, 4; absent = [1, 2, 4]) names the output scales that get a term `voxel_boundary_{f}` = WEIGHT / f x
#   boundary(voxel_f, voxel_target_f, T_f), TRUNCATE_M (a number > 0; absent = 4.0, RayIoU's largest threshold) truncates both
#   distance transforms: T_f = max(1, round(TRUNCATE_M / (VOXEL.RESOLUTION f))) cells.  Needs VOXEL_SEG.ENABLED.
#   VOXEL_SEG.VISIBILITY.{ENABLED,LIDAR_STRIDE,CAMERA_STRIDE} - the sensor-visibility mask of the voxel labels (the reference has
#   none: its labels call every unobserved cell "free").  ENABLED (bool; absent = off: no table, no launch, no new batch key)
#   makes PreProcess add `voxel_visible_label_{1,2,4}`: voxel_label_f with every free cell that no ray of the lidar sweep or the
#   depth camera passes before its first occupied cell set to 255, which the dense voxel losses (cross-entropy, SemScal, GeoScal,
#   Lovasz) and the SSC metrics ignore; evaluation then also logs `{prefix}_Voxel_Unknown_Share`.  LIDAR_STRIDE (an integer >= 1;
#   absent = 1) takes every STRIDE-th azimuth of the range view, CAMERA_STRIDE (an integer >= 1; absent = 2) every STRIDE-th
#   pixel of the full camera frame in both directions.  Needs VOXEL_SEG.ENABLED, refuses VOXEL_SEG.USE_TOP_K.
#   VOXEL_SEG.AGGREGATE.{ENABLED,WINDOW,MIN_FITNESS,ICP_ITERATIONS,ICP_STRIDE,ICP_SEARCH} - fills the cells the visibility mask calls unknown
#   from the neighbouring frames of the same sequence (the reference has none).  ENABLED (bool; absent = off: no launch, no new
#   batch key, no new metric name) makes PreProcess write into `voxel_visible_label_{1,2,4}` the aggregated labels: a cell the
#   frame observed itself stays, every other cell takes what the nearest frame in time (past before future, at most WINDOW frames
#   away - an integer >= 1, absent = 4, a definition and no measured optimum) saw at the place the ego motion carries it to, 255 if
#   none did; evaluation then also logs `{prefix}_Voxel_Filled_Share` and `{prefix}_Voxel_Unknown_Share_Aggregated`.  The ego
#   motion is `batch['voxel_ego_poses']` (b, s - 1, 4, 4) when given, else ICP between consecutive label range views with
#   ICP_ITERATIONS (an integer >= 1; absent = 30) fits on every ICP_STRIDE-th point (an integer >= 1; absent = 4) and the
#   neighbour search ICP_SEARCH (the string brute or grid; absent = brute; grid gives the same poses bit for bit); a link whose
#   fitness is below MIN_FITNESS (a number in [0, 1]; absent = 0.3) or whose registration failed carries nothing
#   (DESIGN.md section 18).  Needs VOXEL_SEG.VISIBILITY.ENABLED, hence VOXEL_SEG.ENABLED and no VOXEL_SEG.USE_TOP_K.
#   MODEL.TRANSFORMER.SENSOR_DROPOUT.{CAMERA,LIDAR} - sensor (modality) dropout of the fusion transformer (the reference has none).
#   Two probabilities (numbers in [0, 1]; absent = 0 = off: no draw, no mask, no new code on the step), CAMERA + LIDAR <= 1: in
#   training mode each SEQUENCE of a batch loses its camera with probability CAMERA, its lidar with probability LIDAR, never
#   both; the dropped sensor's feature map is replaced by zeros and its tokens are hidden as attention keys in all layers
#   (`batch['sensor_drop']`, (b,) with 0 none / 1 camera / 2 lidar, says the same explicitly and in any mode).  DESIGN.md section 19.
EXTENSION_KEYS = ('MODEL.TRANSFORMER.SENSOR_DROPOUT', 'MODEL.TRANSFORMER.SENSOR_DROPOUT.CAMERA', 'MODEL.TRANSFORMER.SENSOR_DROPOUT.LIDAR',
                  'MODEL.CONSTANT_SIZE', 'MODEL.CONSTANT_SIZE.RGB', 'MODEL.CONSTANT_SIZE.LIDAR', 'MODEL.CONSTANT_SIZE.VOXEL',
                  'LOSSES.LIDAR_CD', 'LOSSES.LIDAR_CD.WEIGHT', 'LOSSES.LIDAR_CD.FACTORS',
                  'LOSSES.VOXEL_LOVASZ', 'LOSSES.VOXEL_LOVASZ.WEIGHT', 'LOSSES.VOXEL_LOVASZ.FACTORS',
                  'LOSSES.VOXEL_RENDER', 'LOSSES.VOXEL_RENDER.WEIGHT', 'LOSSES.VOXEL_RENDER.FACTORS', 'LOSSES.VOXEL_RENDER.STRIDE',
                  'LOSSES.VOXEL_RENDER_CLASS', 'LOSSES.VOXEL_RENDER_CLASS.WEIGHT', 'LOSSES.VOXEL_RENDER_CLASS.FACTORS',
                  'LOSSES.VOXEL_RENDER_CLASS.STRIDE',
                  'LOSSES.VOXEL_BOUNDARY', 'LOSSES.VOXEL_BOUNDARY.WEIGHT', 'LOSSES.VOXEL_BOUNDARY.FACTORS', 'LOSSES.VOXEL_BOUNDARY.TRUNCATE_M',
                  'VOXEL_SEG.VISIBILITY', 'VOXEL_SEG.VISIBILITY.ENABLED', 'VOXEL_SEG.VISIBILITY.LIDAR_STRIDE', 'VOXEL_SEG.VISIBILITY.CAMERA_STRIDE',
                  'VOXEL_SEG.AGGREGATE', 'VOXEL_SEG.AGGREGATE.ENABLED', 'VOXEL_SEG.AGGREGATE.WINDOW', 'VOXEL_SEG.AGGREGATE.MIN_FITNESS',
                  'VOXEL_SEG.AGGREGATE.ICP_ITERATIONS', 'VOXEL_SEG.AGGREGATE.ICP_STRIDE', 'VOXEL_SEG.AGGREGATE.ICP_SEARCH')
DEFAULT_CONSTANT_SIZE = {'RGB': (5, 13), 'LIDAR': (1, 16), 'VOXEL': (3, 3, 1)}


def constant_sizes(cfg):
    """(rgb, lidar, voxel) seed sizes of the three decoders: MODEL.CONSTANT_SIZE.* if given, else the reference's constants."""
    cs = cfg.MODEL.get('CONSTANT_SIZE', None) or {}
    out = []
    for k in ('RGB', 'LIDAR', 'VOXEL'):
        v = tuple(int(x) for x in cs.get(k, DEFAULT_CONSTANT_SIZE[k]))
        if len(v) != len(DEFAULT_CONSTANT_SIZE[k]) or min(v) < 1:
            raise ValueError(f'MODEL.CONSTANT_SIZE.{k} must be {len(DEFAULT_CONSTANT_SIZE[k])} positive integers, got {v}')
        out.append(v)
    return tuple(out)


def sensor_dropout(cfg):
    """(camera, lidar) probabilities of sensor dropout: MODEL.TRANSFORMER.SENSOR_DROPOUT.* if given, else (0.0, 0.0) = off"""
    node = cfg.MODEL.TRANSFORMER.get('SENSOR_DROPOUT', None) or {}
    out = []
    for key in ('CAMERA', 'LIDAR'):
        v = node.get(key, 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1:
            raise ValueError(f'MODEL.TRANSFORMER.SENSOR_DROPOUT.{key} must be a number in [0, 1], got {v!r}')
        out.append(float(v))
    if out[0] + out[1] > 1:
        raise ValueError(f'MODEL.TRANSFORMER.SENSOR_DROPOUT: CAMERA + LIDAR must be <= 1 (at most one sensor is dropped per '
                         f'sequence), got {out[0]} + {out[1]}')
    if max(out) > 0 and not cfg.MODEL.TRANSFORMER.ENABLED:
        raise ValueError('MODEL.TRANSFORMER.SENSOR_DROPOUT needs MODEL.TRANSFORMER.ENABLED: the mask is in the fusion transformer')
    return out[0], out[1]


DEFAULT_LIDAR_CD_FACTORS = (2, 4)


def lidar_cd(cfg):
    """(weight, factors) of the Chamfer-distance loss: LOSSES.LIDAR_CD.* if given, else (0.0, (2, 4)); weight 0 = no such term."""
    node = cfg.LOSSES.get('LIDAR_CD', None) or {}
    weight = node.get('WEIGHT', 0.0)
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not weight >= 0:
        raise ValueError(f'LOSSES.LIDAR_CD.WEIGHT must be a number >= 0, got {weight!r}')
    factors = node.get('FACTORS', DEFAULT_LIDAR_CD_FACTORS)
    if not isinstance(factors, (list, tuple)) or any(isinstance(f, bool) or f not in (1, 2, 4) for f in factors) \
            or len(set(factors)) != len(factors):
        raise ValueError(f'LOSSES.LIDAR_CD.FACTORS must be a list of distinct factors drawn from 1, 2, 4, got {factors!r}')
    if weight > 0 and not cfg.LIDAR_RE.ENABLED:
        raise ValueError('LOSSES.LIDAR_CD.WEIGHT > 0 needs LIDAR_RE.ENABLED: the loss is on the lidar reconstruction head')
    return float(weight), tuple(int(f) for f in factors)


DEFAULT_VOXEL_LOVASZ_FACTORS = (1, 2, 4)


def voxel_lovasz(cfg):
    """(weight, factors) of the Lovasz-softmax loss: LOSSES.VOXEL_LOVASZ.* if given, else (0.0, (1, 2, 4)); weight 0 = no such term."""
    node = cfg.LOSSES.get('VOXEL_LOVASZ', None) or {}
    weight = node.get('WEIGHT', 0.0)
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not weight >= 0:
        raise ValueError(f'LOSSES.VOXEL_LOVASZ.WEIGHT must be a number >= 0, got {weight!r}')
    factors = node.get('FACTORS', DEFAULT_VOXEL_LOVASZ_FACTORS)
    if not isinstance(factors, (list, tuple)) or any(isinstance(f, bool) or f not in (1, 2, 4) for f in factors) \
            or len(set(factors)) != len(factors):
        raise ValueError(f'LOSSES.VOXEL_LOVASZ.FACTORS must be a list of distinct factors drawn from 1, 2, 4, got {factors!r}')
    if weight > 0 and not cfg.VOXEL_SEG.ENABLED:
        raise ValueError('LOSSES.VOXEL_LOVASZ.WEIGHT > 0 needs VOXEL_SEG.ENABLED: the loss is on the voxel head')
    return float(weight), tuple(int(f) for f in factors)


DEFAULT_VOXEL_RENDER_FACTORS = (1, 2, 4)
DEFAULT_VOXEL_RENDER_STRIDE = 1


def _rendered_loss(cfg, key, default_factors, default_stride):
    node = cfg.LOSSES.get(key, None) or {}
    weight = node.get('WEIGHT', 0.0)
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not weight >= 0:
        raise ValueError(f'LOSSES.{key}.WEIGHT must be a number >= 0, got {weight!r}')
    factors = node.get('FACTORS', default_factors)
    if not isinstance(factors, (list, tuple)) or any(isinstance(f, bool) or f not in (1, 2, 4) for f in factors) \
            or len(set(factors)) != len(factors):
        raise ValueError(f'LOSSES.{key}.FACTORS must be a list of distinct factors drawn from 1, 2, 4, got {factors!r}')
    stride = node.get('STRIDE', default_stride)
    if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1:
        raise ValueError(f'LOSSES.{key}.STRIDE must be an integer >= 1, got {stride!r}')
    if weight > 0 and not cfg.VOXEL_SEG.ENABLED:
        raise ValueError(f'LOSSES.{key}.WEIGHT > 0 needs VOXEL_SEG.ENABLED: the loss is on the voxel head')
    return float(weight), tuple(int(f) for f in factors), int(stride)


def voxel_render(cfg):
    """(weight, factors, stride) of the rendered first-hit depth loss: LOSSES.VOXEL_RENDER.* if given, else (0.0, (1, 2, 4), 1);
    weight 0 = no such term."""
    return _rendered_loss(cfg, 'VOXEL_RENDER', DEFAULT_VOXEL_RENDER_FACTORS, DEFAULT_VOXEL_RENDER_STRIDE)


DEFAULT_VOXEL_RENDER_CLASS_FACTORS = (1, 2, 4)
DEFAULT_VOXEL_RENDER_CLASS_STRIDE = 1


def voxel_render_class(cfg):
    """(weight, factors, stride) of the rendered first-hit class loss: LOSSES.VOXEL_RENDER_CLASS.* if given, else
    (0.0, (1, 2, 4), 1); weight 0 = no such term.  The rules and texts of voxel_render."""
    return _rendered_loss(cfg, 'VOXEL_RENDER_CLASS', DEFAULT_VOXEL_RENDER_CLASS_FACTORS, DEFAULT_VOXEL_RENDER_CLASS_STRIDE)


DEFAULT_VOXEL_BOUNDARY_FACTORS = (1, 2, 4)
DEFAULT_VOXEL_BOUNDARY_TRUNCATE_M = 4.0            # RayIoU's largest threshold


def voxel_boundary(cfg):
    """(weight, factors, truncate_m) of the distance-transform boundary loss: LOSSES.VOXEL_BOUNDARY.* if given, else
    (0.0, (1, 2, 4), 4.0); weight 0 = no such term.  WEIGHT and FACTORS by the rules and texts of voxel_render; TRUNCATE_M is a
    number > 0, the truncation of both distance transforms in metres (voxel_boundary_cells turns it into cells)."""
    weight, factors, _ = _rendered_loss(cfg, 'VOXEL_BOUNDARY', DEFAULT_VOXEL_BOUNDARY_FACTORS, 1)
    truncate = (cfg.LOSSES.get('VOXEL_BOUNDARY', None) or {}).get('TRUNCATE_M', DEFAULT_VOXEL_BOUNDARY_TRUNCATE_M)
    if isinstance(truncate, bool) or not isinstance(truncate, (int, float)) or not truncate > 0:
        raise ValueError(f'LOSSES.VOXEL_BOUNDARY.TRUNCATE_M must be a number > 0, got {truncate!r}')
    return weight, factors, float(truncate)


def voxel_boundary_cells(cfg, truncate_m, f):
    """the truncation in cells of scale f: max(1, round(TRUNCATE_M / (VOXEL.RESOLUTION f))) - 20, 10, 5 at the defaults"""
    return max(1, int(round(truncate_m / (cfg.VOXEL.RESOLUTION * f))))


DEFAULT_VISIBILITY_LIDAR_STRIDE = 1
DEFAULT_VISIBILITY_CAMERA_STRIDE = 2


def voxel_visibility(cfg):
    """(enabled, lidar stride, camera stride) of the sensor-visibility mask: VOXEL_SEG.VISIBILITY.* if given, else (False, 1, 2);
    off = no table, no launch, no new batch key."""
    node = cfg.VOXEL_SEG.get('VISIBILITY', None) or {}
    enabled = node.get('ENABLED', False)
    if not isinstance(enabled, bool):
        raise ValueError(f'VOXEL_SEG.VISIBILITY.ENABLED must be true or false, got {enabled!r}')
    strides = []
    for key, default in (('LIDAR_STRIDE', DEFAULT_VISIBILITY_LIDAR_STRIDE), ('CAMERA_STRIDE', DEFAULT_VISIBILITY_CAMERA_STRIDE)):
        stride = node.get(key, default)
        if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1:
            raise ValueError(f'VOXEL_SEG.VISIBILITY.{key} must be an integer >= 1, got {stride!r}')
        strides.append(int(stride))
    if enabled and not cfg.VOXEL_SEG.ENABLED:
        raise ValueError('VOXEL_SEG.VISIBILITY.ENABLED needs VOXEL_SEG.ENABLED: the mask is on the labels of the voxel head')
    if enabled and cfg.VOXEL_SEG.USE_TOP_K:
        raise ValueError('VOXEL_SEG.VISIBILITY.ENABLED together with VOXEL_SEG.USE_TOP_K: the top-k cross-entropy runs through a '
                         'different kernel whose treatment of label 255 is not defined')
    return enabled, strides[0], strides[1]


DEFAULT_AGGREGATE_WINDOW = 4                       # frames on each side: a definition, not a measured optimum
DEFAULT_AGGREGATE_MIN_FITNESS = 0.3
DEFAULT_AGGREGATE_ICP_ITERATIONS = 30
DEFAULT_AGGREGATE_ICP_STRIDE = 4
MAX_AGGREGATE_WINDOW = 64                          # the bound of muvo_voxel_pose_chain


def voxel_aggregate(cfg):
    """(enabled, window, min fitness, icp iterations, icp stride) of the fill of unobserved label cells from neighbouring frames:
    VOXEL_SEG.AGGREGATE.* if given, else (False, 4, 0.3, 30, 4); off = no launch, no new batch key, no new metric name."""
    node = cfg.VOXEL_SEG.get('AGGREGATE', None) or {}
    enabled = node.get('ENABLED', False)
    if not isinstance(enabled, bool):
        raise ValueError(f'VOXEL_SEG.AGGREGATE.ENABLED must be true or false, got {enabled!r}')
    window = node.get('WINDOW', DEFAULT_AGGREGATE_WINDOW)
    if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= MAX_AGGREGATE_WINDOW:
        raise ValueError(f'VOXEL_SEG.AGGREGATE.WINDOW must be an integer in 1..{MAX_AGGREGATE_WINDOW}, got {window!r}')
    fitness = node.get('MIN_FITNESS', DEFAULT_AGGREGATE_MIN_FITNESS)
    if isinstance(fitness, bool) or not isinstance(fitness, (int, float)) or not 0 <= fitness <= 1:
        raise ValueError(f'VOXEL_SEG.AGGREGATE.MIN_FITNESS must be a number in [0, 1], got {fitness!r}')
    ints = []
    for key, default in (('ICP_ITERATIONS', DEFAULT_AGGREGATE_ICP_ITERATIONS), ('ICP_STRIDE', DEFAULT_AGGREGATE_ICP_STRIDE)):
        v = node.get(key, default)
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f'VOXEL_SEG.AGGREGATE.{key} must be an integer >= 1, got {v!r}')
        ints.append(int(v))
    if enabled and not voxel_visibility(cfg)[0]:         # its refusals (VOXEL_SEG.ENABLED, USE_TOP_K) are raised by that call
        raise ValueError('VOXEL_SEG.AGGREGATE.ENABLED needs VOXEL_SEG.VISIBILITY.ENABLED: aggregation fills the cells that mask calls unknown')
    return enabled, int(window), float(fitness), ints[0], ints[1]


AGGREGATE_ICP_SEARCHES = ('brute', 'grid')


def voxel_aggregate_icp_search(cfg):
    """the neighbour search of the aggregation's ICP: VOXEL_SEG.AGGREGATE.ICP_SEARCH, 'brute' or 'grid'; absent = 'brute'"""
    node = cfg.VOXEL_SEG.get('AGGREGATE', None) or {}
    search = node.get('ICP_SEARCH', 'brute')
    if not isinstance(search, str) or search not in AGGREGATE_ICP_SEARCHES:
        raise ValueError(f"VOXEL_SEG.AGGREGATE.ICP_SEARCH must be the string 'brute' or 'grid', got {search!r}")
    return search


class CfgNode(dict):
    def __init__(self, init=None):
        super().__init__()
        object.__setattr__(self, '_frozen', False)
        object.__setattr__(self, '_new_allowed', False)
        for k, v in (init or {}).items():
            dict.__setitem__(self, k, CfgNode(v) if isinstance(v, dict) else v)

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        if self._frozen:
            raise AttributeError(f'Attempted to set {name} on a frozen CfgNode')
        self[name] = value

    def _children(self):
        return [v for v in self.values() if isinstance(v, CfgNode)]

    def clone(self):
        return copy.deepcopy(self)

    def freeze(self):
        object.__setattr__(self, '_frozen', True)
        for c in self._children():
            c.freeze()

    def defrost(self):
        object.__setattr__(self, '_frozen', False)
        for c in self._children():
            c.defrost()

    def is_frozen(self):
        return self._frozen

    def set_new_allowed(self, flag):
        object.__setattr__(self, '_new_allowed', flag)
        for c in self._children():
            c.set_new_allowed(flag)

    def convert_to_dict(self):
        return {k: (v.convert_to_dict() if isinstance(v, CfgNode) else v) for k, v in self.items()}

    def _merge(self, other, path=''):
        for k, v in other.items():
            full = f'{path}{k}'
            if k not in self:
                if full in TOLERATED_EXTRA_KEYS:
                    continue
                if self._new_allowed or full in EXTENSION_KEYS:
                    dict.__setitem__(self, k, CfgNode(v) if isinstance(v, dict) else copy.deepcopy(v))
                    continue
                raise KeyError(f'Non-existent config key: {full}')
            cur = self[k]
            if isinstance(cur, CfgNode):
                if not isinstance(v, dict):
                    raise ValueError(f'config key {full} is a section, got {type(v).__name__}')
                cur._merge(v, full + '.')
            else:
                if isinstance(cur, tuple) and isinstance(v, list):
                    v = tuple(v)
                elif isinstance(cur, list) and isinstance(v, tuple):
                    v = list(v)
                elif isinstance(cur, float) and isinstance(v, int) and not isinstance(v, bool):
                    v = float(v)
                dict.__setitem__(self, k, copy.deepcopy(v))

    def merge_from_other_cfg(self, other):
        self._merge(other)

    def merge_from_file(self, path):
        with open(path) as f:
            data = yaml.safe_load(f) or {}
        base = data.pop('_BASE_', None)
        if base:
            if not os.path.isabs(base):
                base = os.path.join(os.path.dirname(os.path.abspath(path)), base)
            self.merge_from_file(base)
        self._merge(data)

    def merge_from_list(self, opts):
        opts = list(opts or [])
        if len(opts) % 2:
            raise ValueError('override list must be KEY VALUE pairs')
        for key, raw in zip(opts[0::2], opts[1::2]):
            node = self
            parts = key.split('.')
            for i, p in enumerate(parts[:-1]):
                if p not in node and '.'.join(parts[:i + 1]) in EXTENSION_KEYS:
                    dict.__setitem__(node, p, CfgNode())
                node = node[p]
            if parts[-1] not in node and key not in EXTENSION_KEYS:
                raise KeyError(f'Non-existent config key: {key}')
            val = raw
            if isinstance(raw, str):
                try:
                    val = yaml.safe_load(raw)
                except yaml.YAMLError:
                    val = raw
            node._merge({parts[-1]: val}, '.'.join(parts[:-1]) + ('.' if len(parts) > 1 else ''))


CN = CfgNode


def _load_defaults():
    with open(os.path.join(_HERE, 'configs', 'defaults.yml')) as f:
        d = yaml.safe_load(f)
    node = CfgNode(d)
    # tuple-typed defaults of the reference
    node.IMAGE['SIZE'] = tuple(node.IMAGE.SIZE)
    node.IMAGE['IMAGENET_MEAN'] = tuple(node.IMAGE.IMAGENET_MEAN)
    node.IMAGE['IMAGENET_STD'] = tuple(node.IMAGE.IMAGENET_STD)
    for k in ('AUGMENTATION_TRANSLATE', 'AUGMENTATION_SCALE', 'AUGMENTATION_SHEAR'):
        node.ROUTE[k] = tuple(node.ROUTE[k])
    return node


_C = _load_defaults()


def get_parser():
    parser = argparse.ArgumentParser(description='World model training')
    parser.add_argument('--config-file', default='', metavar='FILE', help='path to config file')
    parser.add_argument('opts', help='Modify config options using the command-line', default=None,
                        nargs=argparse.REMAINDER)
    return parser


def _extra_keys(known, other, path=''):
    out = []
    for k, v in other.items():
        full = f'{path}.{k}' if path else k
        if k not in known:
            if full not in EXTENSION_KEYS:
                out.append(full)
        elif isinstance(known[k], dict) and isinstance(v, dict):
            out.extend(_extra_keys(known[k], v, full))
    return sorted(out)


def get_cfg(args=None, cfg_dict=None):
    """Defaults, then cfg_dict (unknown keys tolerated with a warning), then args.config_file / args.opts (frozen)."""
    cfg = _C.clone()
    if cfg_dict is not None:
        extra = _extra_keys(cfg, cfg_dict)
        if extra:
            print(f'Warning - the cfg_dict merging into the main cfg has keys that do not exist in main: {extra}')
            cfg.set_new_allowed(True)
        cfg.merge_from_other_cfg(cfg_dict)
    if args is not None:
        if args.config_file:
            cfg.merge_from_file(args.config_file)
        cfg.merge_from_list(args.opts)
        cfg.freeze()
    return cfg


def base_1d_cfg(**overrides):
    """Effective base_1d configuration (defaults <- configs/muvo.yml <- configs/test_base_1d.yml) + overrides."""
    cfg = _C.clone()
    cfg.merge_from_file(os.path.join(_HERE, 'configs', 'test_base_1d.yml'))
    flat = []
    for k, v in overrides.items():
        flat += [k.replace('__', '.'), v]
    cfg.merge_from_list(flat)
    return cfg
