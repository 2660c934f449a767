"""ctypes binding of libmuvo_hip.so (include/muvo_hip.h) + torch.autograd glue.

PyTorch is used here only as plumbing: device memory (torch.empty), the current HIP stream, and the
autograd tape.  Every arithmetic op of the training step is a call into the hand-written gfx950
kernels; there is NO eager/CPU fallback — if the shared library is missing or a call fails, a
RuntimeError is raised (the product path must fail loudly).

Parameter gradients are accumulated by the kernels straight into `param.grad` (pre-allocated, usually a
view into one flat gradient buffer, see muvo_amd/param_store.py); the autograd Functions therefore
return None for parameters and only propagate activation gradients.
"""
import collections
import contextlib
import functools
import ctypes as C
import math
import os
import threading
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get('MUVO_HIP_LIB') or os.path.join(_HERE, 'libmuvo_hip.so')   # MUVO_HIP_LIB: A/B builds on the GPU box
_lib = None
_lock = threading.Lock()

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_ELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4, 5


class ConvDesc(C.Structure):
    _fields_ = [('nd', C.c_int32), ('transposed', C.c_int32), ('N', C.c_int32), ('Cin', C.c_int32), ('Cout', C.c_int32),
                ('in_sz', C.c_int32 * 3), ('out_sz', C.c_int32 * 3), ('ksz', C.c_int32 * 3), ('stride', C.c_int32 * 3),
                ('pad', C.c_int32 * 3), ('dil', C.c_int32 * 3)]


class GemmDesc(C.Structure):
    _fields_ = [('M', C.c_int32), ('N', C.c_int32), ('K', C.c_int32),
                ('sam', C.c_int64), ('sak', C.c_int64), ('sbk', C.c_int64), ('sbn', C.c_int64), ('scm', C.c_int64),
                ('B1', C.c_int32), ('B2', C.c_int32),
                ('a_b1', C.c_int64), ('a_b2', C.c_int64), ('b_b1', C.c_int64), ('b_b2', C.c_int64),
                ('c_b1', C.c_int64), ('c_b2', C.c_int64),
                ('alpha', C.c_float), ('bias_div', C.c_int32), ('act', C.c_int32), ('slope', C.c_float),
                ('mode', C.c_int32)]


class GemmRouteInfo(C.Structure):
    _fields_ = [('kernel', C.c_int32), ('rm', C.c_int32), ('bm', C.c_int32), ('bn', C.c_int32), ('a_lay', C.c_int32),
                ('b_lay', C.c_int32), ('ksplit', C.c_int32), ('grid', C.c_int32 * 3), ('block', C.c_int32)]


class GroupedLinearRouteInfo(C.Structure):
    _fields_ = [('fwd_rm', C.c_int32), ('fwd_grid', C.c_int32), ('dgrad_grid', C.c_int32 * 2), ('wgrad_grid', C.c_int32 * 2)]


class Upsample3dRouteInfo(C.Structure):
    _fields_ = [('kernel', C.c_int32), ('grid', C.c_int32 * 3), ('block', C.c_int32 * 3), ('segs', C.c_int32), ('dseg', C.c_int32)]


class MaxPool2dRouteInfo(C.Structure):
    _fields_ = [('k', C.c_int32), ('load16', C.c_int32), ('v8', C.c_int32), ('grid', C.c_int32 * 3), ('block', C.c_int32 * 3)]


# every exported symbol of include/muvo_hip.h (tests/test_abi.py checks this list against the header)
EXPORTS = [
    'muvo_last_error', 'muvo_abi_version', 'muvo_selftest_mfma', 'muvo_set_deterministic', 'muvo_get_deterministic', 'muvo_reset_accumulators',
    'muvo_conv_set_products', 'muvo_conv_get_products',
    'muvo_conv_set_mode', 'muvo_conv_get_mode', 'muvo_conv_set_bf16x3_min_gflop', 'muvo_conv_pack_sizes', 'muvo_conv_workspace_bytes', 'muvo_conv_kernel_family', 'muvo_conv_kernel_variant', 'muvo_conv_pack_weights', 'muvo_conv_forward', 'muvo_conv_dgrad', 'muvo_conv_prepare_dy', 'muvo_conv_wgrad', 'muvo_bias_grad_nchw',
    'muvo_gemm', 'muvo_gemm_route', 'muvo_grouped_linear_route',
    'muvo_pack_table_item_bytes', 'muvo_conv_pack_table_add', 'muvo_linear_bf16x3_pack_table_add', 'muvo_pack_table_run',
    'muvo_linear_bf16x3_pack_floats', 'muvo_linear_bf16x3_pack', 'muvo_linear_bf16x3_workspace_bytes', 'muvo_linear_bf16x3_split',
    'muvo_linear_bf16x3_forward', 'muvo_linear_bf16x3_dgrad', 'muvo_linear_bf16x3_wgrad',
    'muvo_bn_train_fwd', 'muvo_bn_train_bwd', 'muvo_adain_fwd', 'muvo_adain_bwd',
    'muvo_add_dropout_layernorm_fwd', 'muvo_add_dropout_layernorm_bwd',
    'muvo_act_fwd', 'muvo_act_bwd', 'muvo_dropout', 'muvo_axpby', 'muvo_copy2d', 'muvo_colsum_acc', 'muvo_batchsum',
    'muvo_nchw_to_tokens', 'muvo_tokens_to_nchw', 'muvo_maxpool2d_fwd', 'muvo_maxpool2d_bwd', 'muvo_avgpool_fwd',
    'muvo_avgpool_bwd', 'muvo_upsample3d_x2_fwd', 'muvo_upsample3d_x2_bwd', 'muvo_preprocess_image',
    'muvo_upsample3d_route', 'muvo_maxpool2d_route', 'muvo_softmax_dropout_route',
    'muvo_preprocess_route', 'muvo_divide_scalar', 'muvo_resize_bilinear', 'muvo_resize_nearest_f32',
    'muvo_resize_nearest_u8', 'muvo_softmax_dropout_fwd', 'muvo_softmax_dropout_bwd', 'muvo_gru_fwd', 'muvo_gru_bwd',
    'muvo_rssm_sample_fwd', 'muvo_rssm_sample_bwd',
    'muvo_spatial_loss_fwd', 'muvo_spatial_loss_bwd', 'muvo_spatial_loss_masked_fwd', 'muvo_spatial_loss_masked_bwd', 'muvo_voxel_loss_stats_doubles', 'muvo_voxel_loss_coef_floats',
    'muvo_voxel_loss_fwd', 'muvo_voxel_loss_bwd', 'muvo_l1_rows_fwd', 'muvo_l1_rows_bwd', 'muvo_kl_loss_fwd',
    'muvo_kl_loss_bwd', 'muvo_adamw_step', 'muvo_chamfer_loss_ws_doubles', 'muvo_chamfer_loss_fwd', 'muvo_chamfer_loss_bwd',
    'muvo_ssim_frames', 'muvo_sqdiff_frames', 'muvo_chamfer_sums', 'muvo_ssc_counts', 'muvo_seg_confusion', 'muvo_seg_confusion_index',
    'muvo_frustum_cells', 'muvo_frustum_pool_fwd', 'muvo_frustum_pool_bwd', 'muvo_depth_expectation',
    'muvo_resize_bilinear_bwd', 'muvo_softmax_channel_fwd', 'muvo_softmax_channel_bwd',
    'muvo_range_projection', 'muvo_voxel_grid', 'muvo_seg_ce_fwd', 'muvo_seg_ce_bwd', 'muvo_ssim_maps', 'muvo_ssim_bwd',
    'muvo_instance_labels', 'muvo_pixel_augment', 'muvo_preprocess_route_aug',
    'muvo_split_planes_bytes', 'muvo_split_planes', 'muvo_attention_supported', 'muvo_attention_fwd', 'muvo_attention_bwd',
    'muvo_conv_dgrad_accumulate', 'muvo_conv_forward_moments_supported', 'muvo_conv_forward_moments', 'muvo_adain_fwd_moments',
    'muvo_adain_head_supported', 'muvo_adain_head_fwd', 'muvo_adain_head_bwd', 'muvo_bf3_loop_clock',
    'muvo_grouped_linear_fwd', 'muvo_grouped_linear_bwd', 'muvo_conv_prepare_dy_head', 'muvo_conv_prepare_dy_head_supported',
    'muvo_conv_forward_head_supported', 'muvo_conv_forward_head',
    'muvo_adain_affine', 'muvo_conv_affine_supported', 'muvo_conv_forward_affine', 'muvo_conv_wgrad_affine',
    'muvo_fake_allreduce', 'muvo_resize_bilinear_aa', 'muvo_bn_train_fwd_planes', 'muvo_bn_train_bwd_planes', 'muvo_conv_forward_planes',
    'muvo_stem_conv_supported', 'muvo_stem_conv_forward', 'muvo_stem_conv_wgrad',
    'muvo_rssm_supported', 'muvo_rssm_transposed_floats', 'muvo_rssm_scratch_floats', 'muvo_rssm_forward', 'muvo_rssm_backward',
    'muvo_voxelize_scratch_bytes', 'muvo_voxelize_frames',
    'muvo_birdview_decode_frames', 'muvo_label_components_frames', 'muvo_depth_semantic_decode_frames',
    'muvo_range_projection_frames', 'muvo_voxel_grid_frames',
    'muvo_attention_stream_supported', 'muvo_attention_stream_blocks', 'muvo_attention_stream_fwd', 'muvo_attention_stream_bwd',
    'muvo_voxel_rows_scratch_bytes', 'muvo_voxel_rows_logits', 'muvo_voxel_rows_grid', 'muvo_voxel_rows_write', 'muvo_image_u8',
    'muvo_panel_image', 'muvo_panel_logits', 'muvo_panel_labels', 'muvo_panel_fill', 'muvo_panel_bars', 'muvo_panel_scatter',
    'muvo_panel_voxel_top_logits', 'muvo_panel_voxel_top_grid',
    'muvo_icp_state_doubles', 'muvo_icp_ws_doubles', 'muvo_icp_init', 'muvo_icp_iterate',
    'muvo_icp_grid_bytes', 'muvo_icp_grid_build', 'muvo_icp_iterate_grid',
    'muvo_flow_max_pairs', 'muvo_flow_workspace_bytes', 'muvo_flow_farneback', 'muvo_flow_colour_ws_bytes', 'muvo_flow_colour',
    'muvo_flow_epe_ws_doubles', 'muvo_flow_epe',
    'muvo_raycast_brick_words', 'muvo_raycast_bricks_grid', 'muvo_raycast_bricks_logits', 'muvo_raycast', 'muvo_panel_voxel_view',
    'muvo_ray_iou_ws_doubles', 'muvo_ray_iou_counts',
    'muvo_lovasz_ws_bytes', 'muvo_lovasz_fwd', 'muvo_lovasz_bwd',
    'muvo_render_ws_bytes', 'muvo_render_fwd', 'muvo_render_bwd',
    'muvo_render_class_ws_bytes', 'muvo_render_class_fwd', 'muvo_render_class_bwd',
    'muvo_voxel_edt_ws_bytes', 'muvo_voxel_edt',
    'muvo_voxel_boundary_ws_bytes', 'muvo_voxel_boundary_forward', 'muvo_voxel_boundary_backward',
    'muvo_voxel_cd_ws_bytes', 'muvo_voxel_cd_counts',
    'muvo_bev_instance_ws_bytes', 'muvo_bev_instance_decode', 'muvo_bev_pq_ws_bytes', 'muvo_bev_pq_counts',
    'muvo_visibility_mark', 'muvo_visibility_apply',
    'muvo_voxel_calibration',
    'muvo_voxel_pose_chain', 'muvo_voxel_aggregate',
    'muvo_attention_mask_fwd', 'muvo_attention_mask_bwd', 'muvo_attention_stream_mask_fwd', 'muvo_attention_stream_mask_bwd',
]


def lib():
    """Load the shared library (once). Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(_LIB_PATH):
                    raise RuntimeError(f'{_LIB_PATH} not found: build it with `python -m muvo_amd.build` '
                                       '(there is no fallback path)')
                L = C.CDLL(_LIB_PATH)
                L.muvo_last_error.restype = C.c_char_p
                L.muvo_conv_workspace_bytes.restype = C.c_int64
                L.muvo_linear_bf16x3_workspace_bytes.restype = C.c_int64
                L.muvo_pack_table_item_bytes.restype = C.c_int64
                L.muvo_split_planes_bytes.restype = C.c_int64
                L.muvo_rssm_transposed_floats.restype = C.c_int64
                L.muvo_rssm_scratch_floats.restype = C.c_int64
                L.muvo_voxelize_scratch_bytes.restype = C.c_int64
                L.muvo_voxel_rows_scratch_bytes.restype = C.c_int64
                L.muvo_chamfer_loss_ws_doubles.restype = C.c_int64
                L.muvo_icp_state_doubles.restype = C.c_int64
                L.muvo_icp_ws_doubles.restype = C.c_int64
                L.muvo_icp_grid_bytes.restype = C.c_int64
                for name in ('muvo_flow_max_pairs', 'muvo_flow_workspace_bytes', 'muvo_flow_colour_ws_bytes', 'muvo_flow_epe_ws_doubles',
                             'muvo_raycast_brick_words', 'muvo_ray_iou_ws_doubles', 'muvo_lovasz_ws_bytes', 'muvo_render_ws_bytes',
                             'muvo_render_class_ws_bytes', 'muvo_voxel_edt_ws_bytes', 'muvo_voxel_boundary_ws_bytes', 'muvo_voxel_cd_ws_bytes',
                             'muvo_bev_instance_ws_bytes', 'muvo_bev_pq_ws_bytes'):
                    getattr(L, name).restype = C.c_int64
                for name in EXPORTS:
                    getattr(L, name)  # AttributeError if a declared symbol is missing
                _lib = L
    return _lib


def _ck(rc):
    if rc != 0:
        msg = lib().muvo_last_error().decode()
        reset_accumulators()
        raise RuntimeError(f'muvo_hip error {rc}: {msg}')


_MOMENT_BUFS = []      # weak references to the per-layer float64 moments buffers (conv_moments_buffer)


def reset_accumulators():
    """Error path: buffers that are all-zero between uses by construction - the library's per-stream statistics accumulators and
    the per-layer moments buffers a convolution epilogue fills for the AdaIN that follows - may hold partial sums when an
    exception interrupted a step between producer and consumer.  Called by _ck on every library error and by the trainer when
    a step raises; a no-op cost otherwise (never on the success path)."""
    try:
        if _lib is not None:
            _lib.muvo_reset_accumulators()
        live = []
        for r in _MOMENT_BUFS:
            t = r()
            if t is not None:
                t.zero_()
                live.append(r)
        _MOMENT_BUFS[:] = live
    except Exception:          # the original error is the one to report
        pass


def _st():
    # raw handle of the current PyTorch stream of the current device (fast path: one C call)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _p(t):
    if t is None:
        return C.c_void_p(0)
    assert t.is_cuda and t.is_contiguous(), 'muvo_hip ops need contiguous device tensors'
    return C.c_void_p(t.data_ptr())


def _f(t):
    assert t is None or t.dtype == torch.float32
    return _p(t)


def _i64(v):
    return C.c_int64(int(v))


def _fl(v):
    return C.c_float(float(v))


_weight_epoch = [0]


def bump_weight_epoch():
    """Call after parameters were modified outside torch (the fused AdamW kernel) to invalidate packed weights."""
    _weight_epoch[0] += 1


CONV_F32, CONV_BF16X3, CONV_BF16 = 0, 1, 2     # CONV_BF16: the bf16x3 kernels with ONE product (extension, see include/muvo_hip.h)


def set_conv_mode(mode, min_gflop=None):
    """Select the matrix-pipe arithmetic of the large convolutions (CONV_F32 exact / CONV_BF16X3 split products;
    min_gflop = per-item work below which a phase stays on fp32 MFMA; negative = the library's built-in per-layer policy).  Packed weights and plans depend on it, so both
    caches are invalidated."""
    _ck(lib().muvo_conv_set_mode(CONV_BF16X3 if int(mode) == CONV_BF16 else int(mode)))
    _ck(lib().muvo_conv_set_products(1 if int(mode) == CONV_BF16 else 3))
    if min_gflop is not None:
        _ck(lib().muvo_conv_set_bf16x3_min_gflop(C.c_double(min_gflop)))
    bump_weight_epoch()
    _plan_epoch[0] += 1


def get_conv_mode():
    m = lib().muvo_conv_get_mode()
    return CONV_BF16 if (m == CONV_BF16X3 and lib().muvo_conv_get_products() == 1) else m


_plan_epoch = [0]


def set_deterministic(on=True):
    """Deterministic mode (include/muvo_hip.h: muvo_set_deterministic; MUVO_DETERMINISTIC=1 at start-up): every reduction whose
    result would depend on the arrival order of float / double atomics runs in a fixed order - two runs of the same step are
    bit-identical.  Slower (split-K and pixel-range splits off, ordered workgroup turns, the AdaIN style projections one Linear
    at a time); a debugging aid for parity work.  Plans and packed weights depend on it: both caches are invalidated."""
    global GROUPED_LINEAR
    _ck(lib().muvo_set_deterministic(1 if on else 0))
    GROUPED_LINEAR = (not on) and os.environ.get('MUVO_GROUPED_LINEAR', '1') != '0'   # its data gradient adds 14 layers atomically
    bump_weight_epoch()
    _plan_epoch[0] += 1


def get_deterministic():
    return bool(lib().muvo_get_deterministic())


_join_queued = [False]


def _queue_final_join():
    """Parameter gradients are written by kernels on whatever stream their backward node runs on (branch streams, the
    weight-gradient stream), not by AccumulateGrad nodes, so the autograd engine does not know about them: the first gradient
    write of a backward pass installs an engine callback that makes the stream `backward()` was called on wait for every
    side stream when the pass ends - `p.grad` is then safe to read right after `loss.backward()` like any other gradient."""
    def cb():
        _join_queued[0] = False
        join_side_streams()
    try:
        torch.autograd.Variable._execution_engine.queue_callback(cb)
        _join_queued[0] = True
    except RuntimeError:      # not inside a backward pass
        pass


def grad_of(p):
    """The gradient buffer the kernels accumulate into.  With a ParamStore that is the parameter's slot of the flat gradient
    buffer: if something set p.grad to None (nn.Module.zero_grad(), optimizer.zero_grad(set_to_none=True) of a foreign
    loop) the slot is zeroed and re-bound here, so gradients never land in a detached tensor.  Without a store the tensor is
    allocated on demand.  Frozen parameters (requires_grad=False, OPTIMIZER.FROZEN) get no buffer of their own: the kernels
    that always write a parameter gradient (BatchNorm / LayerNorm backward) add into one shared dump nobody reads."""
    if not p.requires_grad:
        return scratch('frozen_grad_dump', p.numel(), p.device).view(-1)[:p.numel()].view(p.shape)
    if _side_streams and not _join_queued[0]:
        _queue_final_join()
    if p.grad is None:
        view = getattr(p, '_muvo_flat_grad', None)
        if view is not None:
            view.zero_()
            p.grad = view
        else:
            p.grad = torch.zeros_like(p)
    return p.grad


_scratch = {}


def _stream_key(device):
    """Scratch buffers are per (device, HIP stream): independent branches of the model run on side streams (see `branch`) and
    must not share workspaces."""
    device = torch.device(device)
    if device.type != 'cuda':
        return 0
    return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())


def scratch_zeroed(name, nfloats, device):
    """Scratch that is all-zero at allocation; its users (weight-gradient kernels + unpack) leave it all-zero."""
    key = (name, device, torch.float32, _stream_key(device))
    t = _scratch.get(key)
    if t is None or t.numel() < nfloats:
        t = torch.zeros(int(nfloats), device=device, dtype=torch.float32)
        _scratch[key] = t
    return t


def scratch(name, nfloats, device, dtype=torch.float32):
    key = (name, device, dtype, _stream_key(device))
    t = _scratch.get(key)
    if t is None or t.numel() < nfloats:
        t = torch.empty(int(nfloats), device=device, dtype=dtype)
        _scratch[key] = t
    return t


# ------------------------------------------------------------------------------------------------
# Independent sub-networks on side HIP streams.  The route-map encoder (a ResNet-18 on 64 x 64 pixels: ~300 launches of 5-50 us
# that keep a handful of compute units busy), the range-view encoder and two of the three decoders do not depend on what the
# main stream is doing at that time: issued on their own stream they fill the compute units the main stream's kernels leave
# idle.  autograd runs the backward of every node on the stream its forward ran on and synchronises across streams itself;
# parameter gradients are written by the kernels (not by AccumulateGrad nodes), so whoever reads them (optimizer, gradient
# exchange) first calls join_side_streams().  MUVO_STREAMS=0: everything on the current stream.
STREAMS = os.environ.get('MUVO_STREAMS', '1') != '0'
_side_streams = {}
_inputs_ready = {}


# Which logical branch runs on which HIP stream.  Measured on MI355X (profiles/r03i_stream_queues.txt): concurrency pays as long
# as the process keeps AT MOST FOUR streams busy (the current stream included) - a fifth concurrently active queue does not
# serialise gracefully, the step falls from 84 to 104-111 ms - and with the runtime's default of four hardware queues the
# streams of other libraries (RCCL) push ours onto shared queues in an order nobody controls.  So: muvo_amd/__init__.py asks for
# eight hardware queues (GPU_MAX_HW_QUEUES, before HIP initialises) so that every stream below owns one, and the logical
# branches are folded onto a BUDGET of side streams: three alone on the GPU ({encoders, then the range-view decoder} | voxel
# decoder | weight gradients), two when a gradient exchange is attached (its communication stream only carries waits, RCCL's
# own stream is the fourth busy one; the voxel decoder then follows the range-view decoder's stream).  Same-box A/Bs: range-view
# decoder on s0 instead of the main stream 83.3 -> 82.3 ms/step; with a one-rank RCCL group 84.7 -> 83.1.  MUVO_STREAM_MAP
# overrides single entries ("voxel_decoder=main,wgrad=s0").
# (History: the range-view decoder had to leave its side stream for a while - next to the RGB decoder single heads came out with
# a few 16-element groups off by ~1e-2 in about half of all processes.  That was the packed-fp32 instruction finding of
# muvo_amd/build.py; since the library is built without those instructions: 0 of 30 processes, profiles/r03j_lidar_decoder_stream.txt.)
# The ORDER in which the decoders are recorded in forward matters for backward, see models/mile.py.
_STREAM_PLANS = {
    3: {'lidar_encoder': 's0', 'route_encoder': 's0', 'lidar_decoder': 's0', 'voxel_decoder': 's1', 'wgrad': 's2'},
    2: {'lidar_encoder': 's0', 'route_encoder': 's0', 'lidar_decoder': 's0', 'voxel_decoder': 's0', 'wgrad': 's1'},
    1: {'lidar_encoder': 's0', 'route_encoder': 's0', 'lidar_decoder': 'main', 'voxel_decoder': 'main', 'wgrad': 's0'},
    0: {},
}
STREAM_BUDGET = [int(os.environ.get('MUVO_STREAM_BUDGET', '3'))]
STREAM_MAP = dict(kv.split('=') for kv in os.environ.get('MUVO_STREAM_MAP', '').split(',') if '=' in kv)


def set_stream_budget(n):
    """number of side streams the model may use (0..3); SegmentedGradReducer lowers it to 2 when a gradient exchange is attached
    (its communication stream only carries waits, RCCL's own stream is the fourth busy one)"""
    STREAM_BUDGET[0] = max(0, min(3, int(n)))


def side_stream(name, device):
    device = torch.device(device)
    plan = _STREAM_PLANS[max(0, min(3, STREAM_BUDGET[0]))]
    name = STREAM_MAP.get(name, plan.get(name, 'main' if name in _STREAM_PLANS[3] else name))
    if name == 'main':
        return torch.cuda.current_stream(device)
    key = (name, device.index)
    st = _side_streams.get(key)
    if st is None:
        # default: the stream that carries ONLY the weight gradients (leaves of the backward graph: nothing waits for them before
        # the optimizer) runs at low priority - the main stream's chain is the critical path of the step and gets the compute
        # units first (same-box A/Bs, profiles/r04a_priority.txt: 80.9 -> 79.9 and 80.6 -> 80.3 ms/step)
        dflt = 1 if (plan.get('wgrad') == name and list(plan.values()).count(name) == 1) else 0
        st = _side_streams[key] = _new_stream(device, SIDE_PRIORITY.get(name, SIDE_PRIORITY.get('*', dflt)))
    return st


def reserve_memory_pools(device, main_gb=None, side_gb=None):
    """Pre-size PyTorch's caching allocator for a training loop: one large block is allocated and released on the current stream
    and on every side stream that EXISTS (call it after a first step: creating the streams here, in another order, changes their
    hardware-queue assignment), so that each stream's pool serves the step's requests by splitting it.  Without this the pools grow
    while the loop runs - blocks are stream-specific and a block freed on one stream while a kernel of another still reads it
    (record_stream) comes back late, so the allocator keeps calling hipMalloc for dozens of steps.  MUVO_POOL_MAIN_GB (default 32) +
    MUVO_POOL_SIDE_GB (default 12) per side stream; returns the bytes reserved."""
    device = torch.device(device)
    if device.type != 'cuda':
        return 0
    main_gb = float(os.environ.get('MUVO_POOL_MAIN_GB', 32.0)) if main_gb is None else main_gb
    side_gb = float(os.environ.get('MUVO_POOL_SIDE_GB', 12.0)) if side_gb is None else side_gb
    cur = torch.cuda.current_stream(device)
    todo, seen = [(cur, main_gb)], {cur.cuda_stream}
    for (name, idx), st in sorted(_side_streams.items(), key=lambda kv: kv[0][0]):
        if idx == device.index and st.cuda_stream not in seen:
            seen.add(st.cuda_stream)
            todo.append((st, side_gb))
    free = torch.cuda.mem_get_info(device)[0]
    total = 0
    for st, gb in todo:
        nbytes = int(gb * 2 ** 30)
        if nbytes <= 0 or total + nbytes > 0.8 * free:
            continue
        with torch.cuda.stream(st):
            t = torch.empty(nbytes, dtype=torch.uint8, device=device)
            del t
        total += nbytes
    return total


# HIP stream priorities of the side streams (MUVO_SIDE_PRIORITY="*=normal" | "s2=low,s0=normal" ...; physical stream names s0..s2).
# The main stream's chain is the critical path of the step; a low-priority side stream only gets the compute units the main
# stream's launches leave idle.
SIDE_PRIORITY = {k: {'low': 1, 'normal': 0, 'high': -1}.get(v, 0)
                 for k, v in (kv.split('=') for kv in os.environ.get('MUVO_SIDE_PRIORITY', '').split(',') if '=' in kv)}
_hip_rt = [None]


def _new_stream(device, priority=0):
    """a non-blocking HIP stream of the given priority (-1 high, 0 normal, 1 low) as a torch stream object.  torch.cuda.Stream
    only knows 'normal' and 'high' on ROCm, so other priorities are created through the HIP runtime and wrapped."""
    if priority == 0:
        return torch.cuda.Stream(device=device)
    if _hip_rt[0] is None:
        _hip_rt[0] = C.CDLL('libamdhip64.so')
    rt = _hip_rt[0]
    least, greatest = C.c_int(0), C.c_int(0)
    with torch.cuda.device(device):
        if rt.hipDeviceGetStreamPriorityRange(C.byref(least), C.byref(greatest)) != 0:
            return torch.cuda.Stream(device=device)
        prio = least.value if priority > 0 else greatest.value
        h = C.c_void_p(0)
        if rt.hipStreamCreateWithPriority(C.byref(h), C.c_uint(1), C.c_int(prio)) != 0 or not h.value:   # 1 = hipStreamNonBlocking
            return torch.cuda.Stream(device=device)
    return torch.cuda.ExternalStream(h.value, device=device)


def mark_inputs_ready(device):
    """Everything queued so far on the current stream (packed weights, preprocessed batch) is what a branch's first kernels
    depend on: a side stream waits for THIS point, not for the main stream's later work."""
    if STREAMS and torch.device(device).type == 'cuda':
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        _inputs_ready[torch.device(device).index] = ev


def join_side_streams(device=None, into=None):
    """Make `into` (default: the current stream) wait for everything queued on the side streams."""
    _join_queued[0] = False        # (a backward pass that raised never ran its callback)
    if not _side_streams:
        return
    for (name, idx), st in _side_streams.items():
        if device is not None and torch.device(device).index not in (None, idx):
            continue
        (into if into is not None else torch.cuda.current_stream(st.device)).wait_stream(st)


BRANCHES = set(os.environ.get('MUVO_STREAM_BRANCHES', 'route,lidar,decoders,wgrad').split(','))


def stream_event(device):
    """An event at the current point of the current stream (None when side streams are off): `branch(after=...)`."""
    if not (STREAMS and torch.device(device).type == 'cuda'):
        return None
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    return ev


class branch:
    """br = ops.branch('route', 'route', dev, inputs=(x,)); with br: y = br.out(f(x)); ...; br.join() - runs f's kernels on
    the side stream `name` (if the branch group `group` is enabled).  The side stream starts after the event `after`
    (default: the last mark_inputs_ready(); neither: after everything queued on the current stream so far); the current
    stream waits for the branch in join() - call it right before the first consumer of the outputs.  Disabled
    (MUVO_STREAMS=0, group not in MUVO_STREAM_BRANCHES, CPU tensors): a no-op."""

    def __init__(self, group, name, device, inputs=(), after=None):
        device = torch.device(device)
        self.on = STREAMS and group in BRANCHES and device.type == 'cuda'
        self.device, self.name, self.inputs, self.after = device, name, inputs, after
        self.outs, self.joined = [], False

    def __enter__(self):
        if not self.on:
            return self
        self.main = torch.cuda.current_stream(self.device)
        self.side = side_stream(self.name, self.device)
        if self.side == self.main:
            self.on = False
            return self
        ev = self.after if self.after is not None else _inputs_ready.get(self.device.index)
        if ev is None:
            self.side.wait_stream(self.main)
        else:
            self.side.wait_event(ev)
        for t in self.inputs:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(self.side)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def out(self, t):
        """declare a tensor (list / dict of tensors) that leaves the branch: used by the main stream after join()"""
        if self.on:
            for x in (t.values() if isinstance(t, dict) else t if isinstance(t, (list, tuple)) else (t,)):
                if torch.is_tensor(x) and x.is_cuda:
                    self.outs.append(x)
        return t

    def __exit__(self, *exc):
        if self.on:
            self.ctx.__exit__(*exc)
        return False

    def join(self):
        if self.on and not self.joined:
            self.joined = True
            cur = torch.cuda.current_stream(self.device)
            cur.wait_stream(self.side)
            for x in self.outs:
                x.record_stream(cur)


# Weight gradients on their own stream.  In the backward pass of a convolution only the data gradient is on the critical path
# (the next layer's backward needs it); the weight gradient is needed by the optimizer.  Issued on the stream 'wgrad' it runs
# next to the following layers' data-gradient kernels and fills the compute units their tails and small launches leave idle.
# What the two streams share: the split planes of dy - written by the main stream (prepare_dy / dgrad), read by the weight
# gradient - come from a ring of WGRAD_RING buffers, a buffer is rewritten only after the weight gradient that read it has
# finished (event); tensors owned by autograd (x, y, dy, kept planes of x) are marked with record_stream.
WGRAD_STREAM = STREAMS and 'wgrad' in set(os.environ.get('MUVO_STREAM_BRANCHES', 'route,lidar,decoders,wgrad').split(','))
WGRAD_RING = int(os.environ.get('MUVO_WGRAD_RING', '8'))      # same-box A/B, ms/step: 3 slots 86.8, 6: 86.4, 8: 85.95, 12: 85.9 (+8.6 GB of HBM at 8)
_dy_rings = {}


class _DySlot:
    __slots__ = ('t', 'done')

    def __init__(self):
        self.t, self.done = None, None


def _dy_ws_acquire(nfloats, device):
    """next buffer of the current stream's ring of dy-plane workspaces (waits for the weight gradient that last read it)"""
    key = (torch.device(device).index, _stream_key(device))
    ring = _dy_rings.get(key)
    if ring is None:
        ring = _dy_rings[key] = dict(i=0, slots=[_DySlot() for _ in range(WGRAD_RING)])
    ring['i'] = (ring['i'] + 1) % WGRAD_RING
    sl = ring['slots'][ring['i']]
    if sl.done is not None:
        torch.cuda.current_stream(device).wait_event(sl.done)
        sl.done = None
    if sl.t is None or sl.t.numel() < nfloats:
        sl.t = torch.empty(int(nfloats), device=device, dtype=torch.float32)
    return sl


def wgrad_stream(device):
    """the side stream weight gradients are issued on, or None (switched off / CPU / already on it)"""
    if not WGRAD_STREAM or torch.device(device).type != 'cuda':
        return None
    return side_stream('wgrad', device)


# ------------------------------------------------------------------------------------------------
# optional per-kernel-class timing with HIP events on the launch stream (bench.py roofline object)
KERNEL_TIMING = None


class _NoEvent:
    def record(self):
        pass


_NO_EVENT = _NoEvent()


class KernelTiming:
    """only: record events for this kernel class alone (bench.py brackets just the dominant class inside the timed region:
    ~1400 event pairs per step around every conv call cost 2.4 ms/step, ~140 pairs cost 0.2)."""

    def __init__(self, only=None, prealloc=0):
        """prealloc: events created AND recorded once up front.  A torch.cuda.Event gets its HIP event at its first record(), and
        the first few thousand creations of a process grow the runtime's signal pools: bench.py's timed region paid ~100 ms for
        that in its first three steps (105 / 107 / 125 ms against 77) until the pool was filled ahead of it."""
        self.rec = []
        self.only = only
        self.enabled = True          # bench.py brackets every fourth timed step only (each pair costs ~1.5 us of host and queue time)
        self.pool = []
        if prealloc > 0:
            self.pool = [torch.cuda.Event(enable_timing=True) for _ in range(int(prealloc))]
            for e in self.pool:
                e.record()
            torch.cuda.synchronize()

    def bracket(self, cls, flops, launches, tag='', nbytes=0.0):
        if not self.enabled or (self.only is not None and cls.split(':')[0] != self.only):
            return _NO_EVENT, _NO_EVENT
        e0 = self.pool.pop() if self.pool else torch.cuda.Event(enable_timing=True)
        e1 = self.pool.pop() if self.pool else torch.cuda.Event(enable_timing=True)
        self.rec.append((cls, flops, launches, e0, e1, tag, nbytes))
        return e0, e1

    def layer_table(self):
        """Per (kernel class, layer shape) rows sorted by time: the optimisation worklist."""
        torch.cuda.synchronize()
        agg = {}
        for cls, flops, launches, e0, e1, tag, _nb in self.rec:
            a = agg.setdefault((cls, tag), [0.0, 0.0, 0])
            a[0] += e0.elapsed_time(e1) * 1e-3
            a[1] += flops
            a[2] += 1
        rows = sorted(agg.items(), key=lambda kv: -kv[1][0])
        out = [f'{"ms/call":>9} {"calls":>5} {"TFLOP/s":>8} {"GFLOP":>9}  class | layer']
        for (cls, tag), (sec, fl, n) in rows:
            out.append(f'{sec / n * 1e3:9.3f} {n:5d} {fl / max(sec, 1e-12) / 1e12:8.1f} {fl / n / 1e9:9.2f}  {cls} | {tag}')
        return '\n'.join(out)

    def summary(self):
        """(roofline object of the dominant conv kernel family, per-class table).  Times are HIP-event brackets on the
        launch stream around the C-ABI call (they include the small pack/split/unpack helper launches of that call)."""
        torch.cuda.synchronize()
        agg = {}
        for cls, flops, launches, e0, e1, _tag, nb in self.rec:
            a = agg.setdefault(cls, [0.0, 0.0, 0, 0.0])
            a[0] += e0.elapsed_time(e1) * 1e-3
            a[1] += flops
            a[2] += launches
            a[3] += nb
        classes = {k: dict(seconds=v[0], tflop=v[1] / 1e12, launches=v[2], algorithmic_gb=v[3] / 1e9,
                           avg_launch_us=v[0] / max(v[2], 1) * 1e6, tflops=v[1] / max(v[0], 1e-12) / 1e12)
                   for k, v in agg.items()}
        fam = {}
        for k, c in classes.items():
            f = fam.setdefault(k.split(':')[0], dict(seconds=0.0, tflop=0.0, launches=0, gb=0.0))
            f['seconds'] += c['seconds']
            f['tflop'] += c['tflop']
            f['launches'] += c['launches']
            f['gb'] += c['algorithmic_gb']
        mfma = {k: v for k, v in fam.items() if k in PEAK_TFLOPS}
        roof = None
        if mfma:
            dom = max(mfma, key=lambda k: mfma[k]['seconds'])
            f = mfma[dom]
            alg = f['tflop'] / max(f['seconds'], 1e-12)
            mult = MFMA_FLOPS_PER_ALGORITHMIC_FLOP[dom]
            if dom in ('bf16x3_implicit_gemm', 'bf16x3_small_tile') and lib().muvo_conv_get_products() == 1:
                mult = 1.0        # CONV_BF16: one MFMA product per algorithmic product
            roof = dict(bound='mfma', kernel=KERNEL_NAMES[dom], achieved=alg * mult, peak=PEAK_TFLOPS[dom], unit='TFLOP/s',
                        frac=alg * mult / PEAK_TFLOPS[dom], traffic=None, algorithmic_tflops=alg,
                        mfma_flops_per_algorithmic_flop=mult, launches=f['launches'],
                        algorithmic_bytes=f['gb'] * 1e9 / max(f['launches'], 1),
                        algorithmic_bytes_unit='bytes per launch: fp32 operand tensors read once + result written once '
                                               '(4 * (N*Cin*in_pixels + N*Cout*out_pixels + weight elements))',
                        avg_launch_us=f['seconds'] / max(f['launches'], 1) * 1e6,
                        share_of_conv_time=f['seconds'] / max(sum(v['seconds'] for v in fam.values()), 1e-12))
        return roof, classes


FAMILY = {0: 'f32_implicit_gemm', 1: 'bf16x3_implicit_gemm', 2: 'vox_4x4x1', 3: 'heads_valu', 4: 'vox_bf16x3',
          5: 'bf16x3_small_tile', -1: 'unknown'}
KERNEL_NAMES = {'f32_implicit_gemm': 'conv_fwd_kernel / conv_wgrad_kernel (v_mfma_f32_32x32x2_f32)',
                'bf16x3_implicit_gemm': 'conv_bf3_kernel<256,128|128,256> / conv_bf3_wgrad_pp_kernel: eight-wave ping-pong tiles '
                                        '(v_mfma_f32_32x32x16_bf16, 3 products)',
                'bf16x3_small_tile': 'conv_bf3_kernel<64,128> / conv_bf3_wgrad_kernel: four-wave tiles of the same arithmetic',
                'vox_4x4x1': 'vox_conv_kernel / vox_wgrad_kernel (v_mfma_f32_4x4x1_16b_f32)',
                'vox_bf16x3': 'vox_bf3_kernel (v_mfma_f32_16x16x32_bf16, 3 products, rows padded to 16)'}
# dense MFMA peaks from /opt/skills/guides/MI355X_MICROARCH.md
PEAK_TFLOPS = {'f32_implicit_gemm': 157.3, 'bf16x3_implicit_gemm': 2500.0, 'bf16x3_small_tile': 2500.0, 'vox_4x4x1': 157.3,
               'vox_bf16x3': 2500.0}
MFMA_FLOPS_PER_ALGORITHMIC_FLOP = {'f32_implicit_gemm': 1.0, 'bf16x3_implicit_gemm': 3.0, 'bf16x3_small_tile': 3.0,
                                   'vox_4x4x1': 1.0, 'vox_bf16x3': 3.0}




# ================================================================================================ GEMM
def gemm(A, B, Cout, M, N, K, sam, sak, sbk, sbn, scm, bias=None, alpha=1.0, act=ACT_NONE, slope=0.0, mode=0,
         B1=1, B2=1, a_b=(0, 0), b_b=(0, 0), c_b=(0, 0), bias_div=1, a_off=0, b_off=0, c_off=0):
    """Raw strided GEMM on storage pointers (+ element offsets)."""
    d = GemmDesc(M, N, K, sam, sak, sbk, sbn, scm, B1, B2, a_b[0], a_b[1], b_b[0], b_b[1], c_b[0], c_b[1], alpha,
                 bias_div, act, slope, mode)
    pa = C.c_void_p(A.data_ptr() + 4 * a_off)
    pb = C.c_void_p(B.data_ptr() + 4 * b_off)
    pc = C.c_void_p(Cout.data_ptr() + 4 * c_off)
    _ck(lib().muvo_gemm(C.byref(d), pa, pb, pc, _f(bias), _st()))


def act_bwd(y, dy, act, slope):
    """dz = dy * act'(y) from the saved output y of a fused activation; dy itself when there is none"""
    if act == ACT_NONE:
        return dy
    dz = torch.empty_like(dy)
    _ck(lib().muvo_act_bwd(_f(y), _f(dy), _f(dz), _i64(dy.numel()), act, _fl(slope), _st()))
    return dz


def bias_grad_acc(dz, bias, rows, out_f):
    """bias.grad += column sums of the contiguous (rows, out_f) matrix dz"""
    _ck(lib().muvo_colsum_acc(_f(dz), _f(grad_of(bias)), _i64(rows), _i64(out_f), _i64(out_f), _st()))


GEMM_KERNELS = ('tiled', 'skinny_kvec', 'skinny_kcontig', 'skinny_ncontig')


def gemm_route(M, N, K, sam, sak, sbk, sbn, scm, has_bias=False, act=ACT_NONE, mode=0, B1=1, B2=1, a_addr=0, b_addr=0):
    """What `gemm` would launch for these arguments (host code only, no device): dict(kernel, rm, tile, lay, ksplit, grid,
    block).  a_addr / b_addr: the byte addresses of the operands (data_ptr() + 4 * offset); only their alignment counts."""
    d = GemmDesc(M, N, K, sam, sak, sbk, sbn, scm, B1, B2, 0, 0, 0, 0, 0, 0, 1.0, 1, act, 0.0, mode)
    r = GemmRouteInfo()
    _ck(lib().muvo_gemm_route(C.byref(d), C.c_void_p(a_addr), C.c_void_p(b_addr), int(bool(has_bias)), C.byref(r)))
    return {'kernel': GEMM_KERNELS[r.kernel], 'rm': r.rm, 'tile': (r.bm, r.bn), 'lay': (r.a_lay, r.b_lay), 'ksplit': r.ksplit,
            'grid': tuple(r.grid), 'block': r.block}


def grouped_linear_route(m, k, ns):
    """The launches of GroupedLinearFn for (m, k) inputs and layer widths ns (host code only, no device)."""
    r = GroupedLinearRouteInfo()
    _ck(lib().muvo_grouped_linear_route(m, k, len(ns), (C.c_int * len(ns))(*ns), C.byref(r)))
    return {'fwd_rm': r.fwd_rm, 'fwd_grid': r.fwd_grid, 'dgrad_grid': tuple(r.dgrad_grid), 'wgrad_grid': tuple(r.wgrad_grid)}


class LinearFn(torch.autograd.Function):
    """y = act(x @ W^T + b) on the last dim; x (..., in) contiguous.  W grads go to W.grad."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        x = x.contiguous()
        out_f, in_f = weight.shape
        rows = x.numel() // in_f
        y = torch.empty(*x.shape[:-1], out_f, device=x.device, dtype=torch.float32)
        gemm(x, weight, y, rows, out_f, in_f, in_f, 1, 1, in_f, out_f, bias=bias, act=act, slope=slope)
        ctx.act, ctx.slope = act, slope
        ctx.weight, ctx.bias = weight, bias
        ctx.save_for_backward(x, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        out_f, in_f = weight.shape
        rows = x.numel() // in_f
        dz = act_bwd(y, dy.contiguous(), ctx.act, ctx.slope)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            # dx[r][i] = sum_o dz[r][o] W[o][i]
            gemm(dz, weight, dx, rows, in_f, out_f, out_f, 1, in_f, 1, in_f)
        if weight.requires_grad:
            # dW[o][i] += sum_r dz[r][o] x[r][i]
            gemm(dz, x, grad_of(weight), out_f, in_f, rows, 1, out_f, in_f, 1, in_f, mode=1)
            if bias is not None:
                bias_grad_acc(dz, bias, rows, out_f)
        return dx, None, None, None, None


GROUPED_LINEAR = os.environ.get('MUVO_GROUPED_LINEAR', '1') != '0' and os.environ.get('MUVO_DETERMINISTIC', '0') in ('', '0')


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


class GroupedLinearFn(torch.autograd.Function):
    """(y_1, ..., y_L) = (x W_1^T + b_1, ..., x W_L^T + b_L) for L Linear layers that read the same few-row input: the AdaIN
    style projections of a decoder in one launch per pass (csrc/gemm.hip: grouped_linear_*).  args: x, then W_1, b_1, ..."""

    @staticmethod
    def forward(ctx, x, *wb):
        x = x.contiguous()
        ws, bs = list(wb[0::2]), list(wb[1::2])
        m, k = x.shape
        ns = [w.shape[0] for w in ws]
        ys = [torch.empty(m, n, device=x.device, dtype=torch.float32) for n in ns]
        narr = (C.c_int * len(ns))(*ns)
        _ck(lib().muvo_grouped_linear_fwd(_f(x), m, k, len(ws), _ptr_array(ws), _ptr_array(bs), _ptr_array(ys), narr, _st()))
        ctx.ws, ctx.bs, ctx.ns = ws, bs, ns
        ctx.save_for_backward(x)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        x, = ctx.saved_tensors
        ws, bs, ns = ctx.ws, ctx.bs, ctx.ns
        m, k = x.shape
        dys = [torch.zeros(m, n, device=x.device, dtype=torch.float32) if d is None else d.contiguous() for d, n in zip(dys, ns)]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dws = [grad_of(w) if w.requires_grad else None for w in ws]
        dbs = [grad_of(b) if (b is not None and b.requires_grad) else None for b in bs]
        narr = (C.c_int * len(ns))(*ns)
        _ck(lib().muvo_grouped_linear_bwd(_f(x), m, k, len(ws), _ptr_array(ws), _ptr_array(dys), _f(dx) if dx is not None else None,
                                          _ptr_array(dws), _ptr_array(dbs), narr, _st()))
        return (dx,) + (None,) * (2 * len(ws))


def grouped_linear_supported(x, linears):
    if not GROUPED_LINEAR or x.dim() != 2 or not (1 <= len(linears) <= 16):
        return False
    m, k = x.shape
    if m > 24 or k < 64 or k % 4:
        return False
    return all(l.weight.shape[1] == k and l.weight.is_contiguous() and l.weight.data_ptr() % 16 == 0 and
               (l.weight.grad is None or l.weight.grad.data_ptr() % 16 == 0) and
               getattr(l.weight, '_muvo_flat_grad', l.weight).data_ptr() % 16 == 0 for l in linears)


def grouped_linear(x, linears):
    """styles of `linears` (nn.Linear-like modules with .weight / .bias) applied to the same 2-D input, as a tuple"""
    args = []
    for l in linears:
        args += [l.weight, l.bias]
    return GroupedLinearFn.apply(x, *args)


class _LinearPacked:
    __slots__ = ('fwd', 'dgr', 'fwd_key', 'dgr_key', '__weakref__')

    def __init__(self):
        self.fwd = self.dgr = self.fwd_key = self.dgr_key = None


class LinearBf16x3Fn(torch.autograd.Function):
    """The same Linear for token matrices with thousands of rows (transformer encoder) on the bf16x3 implicit-GEMM
    kernels (include/muvo_hip.h: muvo_linear_bf16x3_*): x and dz are split once into bf16 hi/lo planes; forward, data
    gradient and weight gradient all read those planes."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        x = x.contiguous()
        out_f, in_f = weight.shape
        rows = x.numel() // in_f
        L = lib()
        pk = getattr(weight, '_bf3_packed', None)
        if pk is None:
            pk = weight._bf3_packed = _LinearPacked()
        ff, df = C.c_int64(0), C.c_int64(0)
        _ck(L.muvo_linear_bf16x3_pack_floats(in_f, out_f, C.byref(ff), C.byref(df)))
        k = _wkey(weight)
        if pk.fwd is None or pk.fwd_key != k:
            if pk.fwd is None:
                pk.fwd = torch.empty(ff.value, device=x.device, dtype=torch.float32)
            _ck(L.muvo_linear_bf16x3_pack(in_f, out_f, _f(weight), _f(pk.fwd), None, _st()))
            pk.fwd_key = k
            _PACKS.register(_PackEntry('lin', (in_f, out_f), weight, weakref.ref(pk), _plan_epoch[0], _plan_epoch[0]))
        keep = ctx.needs_input_grad[1]      # a backward follows: wgrad reuses the planes of x
        nws = (L.muvo_linear_bf16x3_workspace_bytes(_i64(rows), in_f) + 3) // 4
        ws_x = torch.empty(nws, device=x.device, dtype=torch.float32) if keep else scratch('lin_ws_x', nws, x.device)
        _ck(L.muvo_linear_bf16x3_split(_f(x), _i64(rows), in_f, _p(ws_x), _st()))
        y = torch.empty(*x.shape[:-1], out_f, device=x.device, dtype=torch.float32)
        _ck(L.muvo_linear_bf16x3_forward(_i64(rows), in_f, out_f, _p(ws_x), _f(pk.fwd), _f(bias), _f(y), act, _fl(slope),
                                         _st()))
        ctx.act, ctx.slope, ctx.weight, ctx.bias, ctx.pk = act, slope, weight, bias, pk
        ctx.ws_x = ws_x if keep else None
        ctx.dims = (rows, in_f, out_f, df.value)
        ctx.x_shape = x.shape
        ctx.save_for_backward(y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        weight, bias, pk = ctx.weight, ctx.bias, ctx.pk
        rows, in_f, out_f, df = ctx.dims
        L = lib()
        dy = dy.contiguous()
        dz = act_bwd(y, dy, ctx.act, ctx.slope)
        nws = (L.muvo_linear_bf16x3_workspace_bytes(_i64(rows), out_f) + 3) // 4
        ws_dz = scratch('lin_ws_dz', nws, dy.device)
        _ck(L.muvo_linear_bf16x3_split(_f(dz), _i64(rows), out_f, _p(ws_dz), _st()))
        dx = None
        if ctx.needs_input_grad[0]:
            k = _wkey(weight)
            if pk.dgr is None or pk.dgr_key != k:
                if pk.dgr is None:
                    pk.dgr = torch.empty(df, device=dy.device, dtype=torch.float32)
                _ck(L.muvo_linear_bf16x3_pack(in_f, out_f, _f(weight), None, _f(pk.dgr), _st()))
                pk.dgr_key = k
            dx = torch.empty(ctx.x_shape, device=dy.device, dtype=torch.float32)
            _ck(L.muvo_linear_bf16x3_dgrad(_i64(rows), in_f, out_f, _p(ws_dz), _f(pk.dgr), _f(dx), _st()))
        if weight.requires_grad:
            sc = scratch_zeroed('lin_wgrad', out_f * in_f, dy.device)
            _ck(L.muvo_linear_bf16x3_wgrad(_i64(rows), in_f, out_f, _p(ctx.ws_x), _p(ws_dz), _f(sc), _f(grad_of(weight)),
                                           _st()))
            if bias is not None:
                bias_grad_acc(dz, bias, rows, out_f)
        return dx, None, None, None, None


LINEAR_BF16X3_MIN_ROWS = int(os.environ.get('MUVO_LINEAR_BF16X3_MIN_ROWS', '2048'))


def linear(x, weight, bias=None, act=ACT_NONE, slope=0.0):
    out_f, in_f = weight.shape
    if (x.numel() // in_f >= LINEAR_BF16X3_MIN_ROWS and in_f % 8 == 0 and out_f % 16 == 0 and in_f >= 64 and out_f >= 64
            and get_conv_mode() == CONV_BF16X3):
        return LinearBf16x3Fn.apply(x, weight, bias, act, slope)
    return LinearFn.apply(x, weight, bias, act, slope)


# ================================================================================================ conv
_PLAN_FIELDS = ('desc', 'out_sz', 'pack_fwd', 'pack_dgrad', 'geom', 'n', 'in_sz', 'oshape', 'pack_key',
                'ws_fwd_x', 'ws_dgrad_dy', 'ws_wgrad_x', 'ws_wgrad_dy', 'fam_fwd', 'fam_dgrad', 'fam_wgrad',
                'dy_planes', 'dy_planes_floats', 'timing', 'answers')


class ConvPlan(collections.namedtuple('ConvPlan', _PLAN_FIELDS)):
    """What the library answers about one convolution at one batch and input size in the current mode (ConvGeom.plan makes one
    per (n, in_sz, plan epoch)): descriptor, sizes, the kernel family of each direction (include/muvo_hip.h:
    muvo_conv_kernel_family) and what the dispatch derives from them.  Workspace sizes are bytes (muvo_conv_workspace_bytes):
    ws_fwd_x / ws_wgrad_x the split copy of x that forward / the weight gradient read, ws_dgrad_dy / ws_wgrad_dy the split
    copy of dy that the data / weight gradient read; pack_fwd / pack_dgrad are floats (muvo_conv_pack_sizes).  A tuple with named
    fields, the descriptor first: plan[0] is what a caller that only wants C.byref(descriptor) takes."""
    __slots__ = ()

    def __new__(cls, geom, n, in_sz, epoch):
        L = lib()
        out_sz = geom.out_size(in_sz)
        d = ConvDesc(geom.nd, geom.transposed, n, geom.cin, geom.cout, (C.c_int32 * 3)(*in_sz),
                     (C.c_int32 * 3)(*out_sz), (C.c_int32 * 3)(*geom.ksz), (C.c_int32 * 3)(*geom.stride),
                     (C.c_int32 * 3)(*geom.pad), (C.c_int32 * 3)(*geom.dil))
        ff, df = C.c_int64(0), C.c_int64(0)
        _ck(L.muvo_conv_pack_sizes(C.byref(d), C.byref(ff), C.byref(df)))
        ws = [L.muvo_conv_workspace_bytes(C.byref(d), op) for op in (0, 1, 2, 3)]
        if min(ws) < 0:
            raise RuntimeError(f'muvo_hip error: {L.muvo_last_error().decode()}')
        fam = [L.muvo_conv_kernel_family(C.byref(d), op) for op in (0, 1, 2)]
        ws_fwd_x, ws_dgrad_dy, ws_wgrad_x, ws_wgrad_dy = ws
        fam_fwd, fam_dgrad, fam_wgrad = fam
        # both gradient kernels read dy through channels-last split planes (one buffer of dy_planes_floats serves both)
        dy_planes = fam_dgrad == 1 and fam_wgrad == 1 and ws_dgrad_dy > 0 and ws_wgrad_dy > 0
        # KernelTiming.bracket arguments per direction.  Class label: family 1 launches on the four-wave small tiles are
        # reported as their own class (5), and so are the stem kernels (csrc/conv_stem.hip, one launch each).  Launches: a
        # transposed convolution is one launch per stride phase in forward and weight gradient, a strided one in the data gradient
        label = [FAMILY[5 if (f == 1 and L.muvo_conv_kernel_variant(C.byref(d), op) == 0) else f] for op, f in enumerate(fam)]
        phases, taps, pix_in, pix_out = math.prod(geom.stride), math.prod(geom.ksz), math.prod(in_sz), math.prod(out_sz)
        flops = 2.0 * n * geom.cin * geom.cout * taps * (pix_in if geom.transposed else pix_out)
        # algorithmic HBM bytes of one operation (forward, data gradient or weight gradient alike): both activation tensors and
        # the weight, fp32, each touched once
        nbytes = 4.0 * (n * geom.cin * pix_in + n * geom.cout * pix_out + geom.cin * geom.cout * taps)
        tag = (f'{"convT" if geom.transposed else "conv"}{geom.nd}d {geom.cin}->{geom.cout} k{geom.ksz} s{geom.stride} '
               f'n{n} in{tuple(in_sz)}')
        rest = (tag, nbytes)
        timing = {'fwd': (label[0] + ':fwd', flops, phases if geom.transposed else 1) + rest,
                  'dgrad': (label[1] + ':dgrad', flops, 1 if geom.transposed else phases) + rest,
                  'wgrad': (label[2] + ':wgrad', flops, phases if geom.transposed else 1) + rest,
                  'stem_fwd': ('bf16x3_small_tile:fwd', flops, 1) + rest,
                  'stem_wgrad': ('bf16x3_small_tile:wgrad', flops, 1) + rest}
        return super().__new__(cls, d, out_sz, ff.value, df.value, geom, n, in_sz,
                               oshape=(n, geom.cout) + (out_sz if geom.nd == 3 else out_sz[1:]),
                               pack_key=(in_sz, epoch),   # what a packed copy of the weight was made for (its layout is batch-independent)
                               ws_fwd_x=ws_fwd_x, ws_dgrad_dy=ws_dgrad_dy, ws_wgrad_x=ws_wgrad_x, ws_wgrad_dy=ws_wgrad_dy,
                               fam_fwd=fam_fwd, fam_dgrad=fam_dgrad, fam_wgrad=fam_wgrad, dy_planes=dy_planes,
                               dy_planes_floats=(max(ws_dgrad_dy, ws_wgrad_dy) + 3) // 4, timing=timing, answers={})

    def supports(self, query, *args):
        """the library's yes / no to `query` (the name of a muvo_*_supported function of the descriptor and args), asked once"""
        key = (query,) + args
        ok = self.answers.get(key)
        if ok is None:
            ok = self.answers[key] = bool(getattr(lib(), query)(C.byref(self.desc), *args))
        return ok


class ConvGeom:
    """Static geometry of a conv layer (everything but the batch/input size)."""

    def __init__(self, nd, transposed, cin, cout, ksz, stride=1, pad=0, dil=1, out_pad=0):
        def t3(v):
            v = (v,) * nd if isinstance(v, int) else tuple(v)
            return (1,) * (3 - nd) + v if nd == 2 and len(v) == 2 else v
        self.nd, self.transposed, self.cin, self.cout = nd, int(transposed), cin, cout
        self.ksz, self.stride, self.dil = t3(ksz), t3(stride), t3(dil)
        p, op = t3(pad), t3(out_pad)
        if nd == 2:
            p = (0,) + p[1:]
            op = (0,) + op[1:]
            self.stride = (1,) + self.stride[1:]
            self.dil = (1,) + self.dil[1:]
        self.pad, self.out_pad = p, op
        self._plans = {}

    def out_size(self, in_sz):
        o = []
        for a in range(3):
            if not self.transposed:
                o.append((in_sz[a] + 2 * self.pad[a] - self.dil[a] * (self.ksz[a] - 1) - 1) // self.stride[a] + 1)
            else:
                o.append((in_sz[a] - 1) * self.stride[a] - 2 * self.pad[a] + self.dil[a] * (self.ksz[a] - 1) + 1 +
                         self.out_pad[a])
        return tuple(o)

    def plan(self, n, in_sz):
        """the ConvPlan for batch n and input size in_sz ((D, H, W); (1, H, W) for a 2-d layer) in the current mode"""
        key = (n, in_sz, _plan_epoch[0])
        pl = self._plans.get(key)
        if pl is None:
            pl = self._plans[key] = ConvPlan(self, n, in_sz, key[2])
        return pl

    def plan_for(self, x):
        """the plan for the input tensor x, or for its shape (N, Cin, spatial...)"""
        shape = getattr(x, 'shape', x)
        return self.plan(shape[0], tuple(shape[2:]) if self.nd == 3 else (1,) + tuple(shape[2:]))


class _PackedWeights:
    """Per-layer K-major packed copies of the weight, refreshed when the weight changed."""

    def __init__(self):
        self.fwd = self.dgr = None
        self.fwd_key = self.dgr_key = None
        self.fwd_plan = self.dgr_plan = None     # ConvPlan.pack_key the copy was packed for


def _wkey(w):
    return (w._version, _weight_epoch[0], w.data_ptr())


def _is_alias(buf, weight):
    return buf is not None and buf.data_ptr() == weight.data_ptr()


_PACKED_ATTRS = (('fwd', 'fwd_key', 'fwd_plan'), ('dgr', 'dgr_key', 'dgr_plan'))


def _packed_weight(plan, packed, weight, dgrad):
    """The packed copy of `weight` that one direction of `plan` reads (dgrad 0: forward and weight gradient, 1: data gradient),
    held by `packed` and made current here: (re)allocated, and packed again when the weight or the plan changed.  Only the
    forward copy registers the layer for the batched repack (repack_all refreshes whichever copies a registered layer has)."""
    a_buf, a_key, a_plan = _PACKED_ATTRS[dgrad]
    buf, key, k = getattr(packed, a_buf), getattr(packed, a_key), _wkey(weight)
    if (plan.fam_dgrad if dgrad else plan.fam_fwd) == 3 and weight.is_contiguous():
        # The 1x1 head kernels (muvo_conv_kernel_family == 3, conv_pw.hip) read the weight in PyTorch's layout: their "packed
        # copy" is the parameter itself - no device-to-device copy per head, direction and optimizer step (18 launches per
        # step at base_1d)
        buf = weight.detach().view(-1)
    else:
        size = plan.pack_dgrad if dgrad else plan.pack_fwd
        if buf is None or buf.numel() < size or _is_alias(buf, weight):
            buf, key = torch.empty(size, device=weight.device, dtype=torch.float32), None
        if key == k and getattr(packed, a_plan) == plan.pack_key:
            return buf
        _ck(lib().muvo_conv_pack_weights(C.byref(plan.desc), _f(weight), None if dgrad else _f(buf), _f(buf) if dgrad else None,
                                         _st()))
        if not dgrad:
            _PACKS.register(_PackEntry('conv', plan.desc, weight, weakref.ref(packed), plan.pack_key, plan.pack_key[1]))
    setattr(packed, a_buf, buf)
    setattr(packed, a_key, k)
    setattr(packed, a_plan, plan.pack_key)
    return buf


# ------------------------------------------------------------------------------------------------
# Batched weight packing (include/muvo_hip.h: muvo_pack_table_*).  Layers register themselves the first time they pack;
# repack_all() (called once per training forward) refreshes every registered copy that already exists with ONE launch and
# marks it current, so the per-layer staleness checks in ConvFn / LinearBf16x3Fn find nothing to do.
# One registered layer.  kind 'conv': desc is the ConvDesc, pack_key the ConvPlan.pack_key; kind 'lin': desc is (in_features,
# out_features), pack_key the plan epoch.  holder: weak reference to the layer's packed-copy holder; epoch: the plan epoch of the copies
_PackEntry = collections.namedtuple('_PackEntry', 'kind desc weight holder pack_key epoch')


class _PackRegistry:
    def __init__(self):
        self.entries, self.seen = [], set()
        self.sig, self.dev, self.n, self.nblk, self.batched = None, None, 0, 0, []

    def register(self, entry):
        key = (id(entry.holder()), entry.pack_key)
        if key not in self.seen:
            self.seen.add(key)
            self.entries.append(entry)


_PACKS = _PackRegistry()
_PACK_BATCH = os.environ.get('MUVO_PACK_BATCH', '1') != '0'


def repack_all():
    flush_bn_counters()
    R = _PACKS
    if not R.entries or not _PACK_BATCH:
        return
    L = lib()
    ptr = lambda t: 0 if t is None else t.data_ptr()
    # drop layers that no longer exist and copies that belong to an earlier plan epoch (conv mode / policy change: their
    # buffers are re-sized lazily by the layer itself, which then registers again)
    live = [(e, e.holder()) for e in R.entries]
    live = [(e, pk) for e, pk in live if pk is not None and e.epoch == _plan_epoch[0]]
    if len(live) != len(R.entries):
        R.entries = [e for e, _ in live]
        R.seen = {(id(pk), e.pack_key) for e, pk in live}
        R.sig = None
    if not R.entries:
        return
    sig = tuple((ptr(pk.fwd), ptr(pk.dgr), e.weight.data_ptr()) for e, pk in live)
    if sig != R.sig:
        item = L.muvo_pack_table_item_bytes()
        cap = 16 * len(live) + 8
        host = torch.zeros(cap * item, dtype=torch.uint8)
        n, nblk = C.c_int(0), C.c_int64(0)
        R.batched = []
        for e, pk in live:
            if pk.fwd is None and pk.dgr is None:
                continue
            if _is_alias(pk.fwd, e.weight) or _is_alias(pk.dgr, e.weight):      # 1x1 heads: the kernels read the parameter itself
                continue
            if e.kind == 'conv':
                rc = L.muvo_conv_pack_table_add(C.c_void_p(host.data_ptr()), cap, C.byref(n), C.byref(nblk), C.byref(e.desc),
                                                _f(e.weight), _f(pk.fwd), _f(pk.dgr))
            else:
                rc = L.muvo_linear_bf16x3_pack_table_add(C.c_void_p(host.data_ptr()), cap, C.byref(n), C.byref(nblk),
                                                         e.desc[0], e.desc[1], _f(e.weight), _f(pk.fwd), _f(pk.dgr))
            if rc == 0:
                R.batched.append(e)
            elif rc != 1:
                _ck(rc)
        R.n, R.nblk = n.value, nblk.value
        R.dev = host[:max(R.n, 1) * item].to(live[0][0].weight.device)
        R.sig = sig
    if R.n:
        _ck(L.muvo_pack_table_run(C.c_void_p(R.dev.data_ptr()), R.n, _i64(R.nblk), _st()))
        for e in R.batched:
            pk = e.holder()
            if pk is None:
                continue
            k = _wkey(e.weight)
            if pk.fwd is not None:
                pk.fwd_key = k
            if pk.dgr is not None:
                pk.dgr_key = k
            if e.kind == 'conv':
                pk.fwd_plan = e.pack_key if pk.fwd is not None else pk.fwd_plan
                pk.dgr_plan = e.pack_key if pk.dgr is not None else pk.dgr_plan


_KEEP_WS = os.environ.get('MUVO_KEEP_WS', '1') != '0'


def _bracket(plan, direction):
    """Opens the timing bracket around one library call of `plan` (direction: a key of ConvPlan.timing) and returns the closing
    event.  The call sites test KERNEL_TIMING themselves, so that a site costs one global read when timing is off:
        e1 = _bracket(plan, 'fwd') if KERNEL_TIMING is not None else None; ...; if e1 is not None: e1.record()"""
    e0, e1 = KERNEL_TIMING.bracket(*plan.timing[direction])
    e0.record()
    return e1


@contextlib.contextmanager
def _on_wgrad_stream(wst, device, reads, dy_slot=None):
    """Runs the body on the weight-gradient stream wst (on the current stream if wst is None or is the current one).  Everything
    the body reads is queued on the current stream by now: wst starts behind that point, and the tensors in `reads` (None
    entries skipped) are kept from being reused before wst is done with them.  dy_slot: the ring slot of dy planes the body
    reads (_dy_ws_acquire), released by an event behind the body's work."""
    cur = torch.cuda.current_stream(device)
    if wst is None or wst == cur:
        yield
        return
    wst.wait_stream(cur)
    for t in reads:
        if t is not None:
            t.record_stream(wst)
    with torch.cuda.stream(wst):
        yield
        if dy_slot is not None:
            dy_slot.done = torch.cuda.Event()
            dy_slot.done.record(wst)


class _DyWorkspace:
    """The dy planes both gradient kernels of one backward call read: with the weight gradient on its own stream (wst) a ring
    buffer (one slot per backward call), otherwise the stream's scratch."""
    __slots__ = ('wst', 'device', 'slot')

    def __init__(self, wst, device):
        self.wst, self.device, self.slot = wst, device, None

    def get(self, nfloats):
        if self.wst is None:
            return scratch('conv_ws_dy', nfloats, self.device)
        if self.slot is None:
            self.slot = _dy_ws_acquire(nfloats, self.device)
        assert self.slot.t.numel() >= nfloats
        return self.slot.t


class ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, geom, packed, act, slope, act_bwd_fused=False, moments=None, aff_src=None, aff=None):
        # aff given: x is the placeholder output of a lazy AdaIN (AdaINFn, lazy=True), the real operand is aff * aff_src + shift,
        # applied by the kernels while they stage aff_src (muvo_conv_forward_affine / muvo_conv_wgrad_affine)
        ctx.aff = aff
        if aff is not None:
            x = aff_src
        # split planes that came with the tensor (written by its producer: BNActFn with planes=True): (workspace, stream key)
        xp = getattr(x, '_muvo_planes', None)
        x_ph = getattr(x, '_muvo_planes_only', False)
        if not x_ph:
            x = x.contiguous()
        plan = geom.plan_for(x)
        hf = getattr(ctx, '_head_fwd', None)      # ConvHeadFn: (head weight, head bias, logits) of a head fused into the epilogue
        ctx.geom, ctx.packed, ctx.act, ctx.slope, ctx.act_bwd_fused = geom, packed, act, slope, act_bwd_fused
        ctx.weight, ctx.bias = weight, bias
        # the 7x7 stride-2 stems of the ResNet-18 trunks: direct convolution on bf16x3 products from the fp32 parameter itself
        # (csrc/conv_stem.hip); only where the arithmetic mode is bf16x3 and the input needs no gradient
        ctx.stem = bool(plan.supports('muvo_stem_conv_supported') and get_conv_mode() != CONV_F32 and bias is None
                        and act == ACT_NONE and moments is None and aff is None and not x_ph and not ctx.needs_input_grad[0]
                        and hf is None and weight.is_contiguous())
        if ctx.stem:
            return ConvFn._stem_forward(ctx, plan, x, weight)
        wp = _packed_weight(plan, packed, weight, 0)
        y = torch.empty(plan.oshape, device=x.device, dtype=torch.float32)
        e1 = _bracket(plan, 'fwd') if KERNEL_TIMING is not None else None
        use_xp = (xp is not None and plan.ws_fwd_x > 0 and plan.fam_fwd == 1 and hf is None and aff is None
                  and moments is None and xp[1] == _stream_key(x.device) and xp[0].numel() * 4 >= plan.ws_fwd_x)
        ws = ConvFn._forward_workspace(ctx, plan, x, xp[0] if use_xp else None, x_ph)
        L, d = lib(), C.byref(plan.desc)
        if hf is not None:
            _ck(L.muvo_conv_forward_head(d, _f(x), _f(wp), _f(bias), _f(y), act, _fl(slope), _p(ws),
                                         _f(hf[0]), _f(hf[1]), hf[0].shape[0], _f(hf[2]), _st()))
        elif aff is not None:
            _ck(L.muvo_conv_forward_affine(d, _f(x), _f(aff), _f(wp), _f(bias), _f(y), act, _fl(slope), _p(moments), _st()))
        elif moments is not None:     # instance-norm statistics of y from the epilogue registers (voxel bf16x3 kernels)
            _ck(L.muvo_conv_forward_moments(d, _f(x), _f(wp), _f(bias), _f(y), act, _fl(slope), _p(moments), _st()))
        elif use_xp:
            _ck(L.muvo_conv_forward_planes(d, None if x_ph else _f(x), _f(wp), _f(bias), _f(y), act, _fl(slope), _p(ws), 1, _st()))
        else:
            _ck(L.muvo_conv_forward(d, _f(x), _f(wp), _f(bias), _f(y), act, _fl(slope), _p(ws), _st()))
        if e1 is not None:
            e1.record()
        ctx.save_for_backward(x, y if (act != ACT_NONE and not act_bwd_fused) else None)
        return y

    @staticmethod
    def _forward_workspace(ctx, plan, x, planes, x_ph):
        """The split copy of x the forward kernel reads (None: this family reads x itself).  planes: the copy that came with x
        where the kernel can read it as it is; x_ph: x has no fp32 values, only those planes.  Leaves in ctx.ws_x the copy
        that the weight gradient reuses."""
        wgrad_follows = ctx.needs_input_grad[1]   # grad mode is off inside forward: needs_input_grad says whether a backward follows
        if x_ph and not (planes is not None and (plan.ws_wgrad_x > 0 or not wgrad_follows)):
            raise RuntimeError('muvo_hip: a planes-only tensor (BNActFn keep_f32=False) reached a convolution that needs its fp32 values')
        if planes is not None:
            ws = planes
            keep_ws = plan.ws_wgrad_x > 0 and wgrad_follows and (_KEEP_WS or x_ph)
        else:
            keep_ws = plan.ws_fwd_x > 0 and plan.ws_wgrad_x > 0 and wgrad_follows and _KEEP_WS
            if keep_ws:
                ws = torch.empty((plan.ws_fwd_x + 3) // 4, device=x.device, dtype=torch.float32)
            else:
                ws = scratch('conv_ws', (plan.ws_fwd_x + 3) // 4, x.device) if plan.ws_fwd_x else None
        ctx.ws_x = ws if keep_ws else None
        ctx.x_is_placeholder = x_ph
        return ws

    @staticmethod
    def _stem_forward(ctx, plan, x, weight):
        y = torch.empty(plan.oshape, device=x.device, dtype=torch.float32)
        e1 = _bracket(plan, 'stem_fwd') if KERNEL_TIMING is not None else None
        _ck(lib().muvo_stem_conv_forward(C.byref(plan.desc), _f(x), _f(weight), None, _f(y), 0, _st()))
        if e1 is not None:
            e1.record()
        ctx.ws_x, ctx.x_is_placeholder = None, False
        ctx.save_for_backward(x, None)
        return y

    @staticmethod
    def _stem_backward(ctx, plan, x, dy):
        # stem: only the weight gradient exists (the input image needs none); on the weight-gradient stream like the others
        weight = ctx.weight
        if not (weight.requires_grad and dy is not None):
            return
        dy = dy.contiguous()
        gw = grad_of(weight)
        with _on_wgrad_stream(wgrad_stream(x.device), x.device, (x, dy)):
            e1 = _bracket(plan, 'stem_wgrad') if KERNEL_TIMING is not None else None
            _ck(lib().muvo_stem_conv_wgrad(C.byref(plan.desc), _f(x), _f(dy), _f(gw), _st()))
            if e1 is not None:
                e1.record()

    @staticmethod
    def backward(ctx, dy):
        return ConvFn._backward(ctx, dy, None)

    @staticmethod
    def _backward(ctx, dy, head):
        """head: None, or (dlogits, head_weight (CO, Cout), head_bias, head_wgrad) of a 1x1 output head that reads this layer's
        output: its data gradient W_head^T dlogits is added to dy inside the split pass (muvo_conv_prepare_dy_head) — dy may
        then be None (the head is the only consumer); head_wgrad() runs the head's own weight-gradient pass."""
        x, y = ctx.saved_tensors
        # the plan of the current epoch, not forward's: the library picks its kernels from its mode at the time of the call
        plan = ctx.geom.plan_for(x)
        if getattr(ctx, 'stem', False):
            ConvFn._stem_backward(ctx, plan, x, dy)
            return (None,) * 11
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.weight.requires_grad
        # both gradient kernels read dy through the channels-last split planes: one fused pass makes them from (y, dy)
        # together with the activation derivative and the bias gradient
        fused_dy = plan.dy_planes and need_dx and need_dw
        dy_ws = _DyWorkspace(wgrad_stream(x.device) if need_dw else None, x.device)
        dz, planes = ConvFn._resolve_dy(ctx, plan, x, y, dy, head, fused_dy, dy_ws)
        dx = None
        if need_dx:
            dx, planes = ConvFn._data_grad(ctx, plan, x, dz, planes, fused_dy, dy_ws)
        if need_dw:
            # the planes hold dy only if the data gradient (or the fused pass before it) split dy into them
            ConvFn._weight_grad(ctx, plan, x, y, dz, planes, need_dx and plan.ws_dgrad_dy > 0, fused_dy, dy_ws)
        return (dx,) + (None,) * 10

    @staticmethod
    def _resolve_dy(ctx, plan, x, y, dy, head, fused_dy, dy_ws):
        """-> (dz, planes): the gradient at the convolution's result (before its activation) as the gradient kernels take it.
        planes: its split planes where they exist already, else None.  Where they exist the bf16x3 kernels (fused_dy says both
        directions run on them) read nothing else, and dz is only some valid pointer."""
        dyp = getattr(dy, '_muvo_planes', None) if dy is not None else None     # dy arrives as split planes (BNActFn.backward)
        if dy is not None and dyp is None:
            dy = dy.contiguous()
        use_act = ctx.act != ACT_NONE and not ctx.act_bwd_fused
        if head is not None and not (fused_dy and plan.supports('muvo_conv_prepare_dy_head_supported', head[1].shape[0])):
            # no fused preamble for this shape: materialise the head's data gradient (dy + W_head^T dlogits)
            gl, head_w, _, head_wgrad = head
            hd = torch.einsum('nk...,kc->nc...', gl, head_w.view(head_w.shape[0], -1))
            dy = hd.contiguous() if dy is None else dy + hd
            head_wgrad()
            head = None
        if dyp is not None:
            if not (fused_dy and head is None and ctx.bias is None and not use_act
                    and dyp[0].numel() >= plan.dy_planes_floats and dyp[1] == _stream_key(x.device)):
                raise RuntimeError('muvo_hip: a gradient that exists only as split planes reached a convolution backward that cannot read them')
            return dyp[0], dyp[0]          # (dz: pointer stand-in)
        if fused_dy:
            return ConvFn._split_dy(ctx, plan, x, y, dy, head, use_act, dy_ws.get(plan.dy_planes_floats))
        # (dy itself: no activation, or its derivative was already chained by the consumer's backward)
        return act_bwd(y, dy, ctx.act if use_act else ACT_NONE, ctx.slope), None

    @staticmethod
    def _split_dy(ctx, plan, x, y, dy, head, use_act, planes):
        """The fused split pass: planes <- split(act'(y) * (dy + the head's data gradient)), bias gradient accumulated.
        -> (pointer stand-in for dz, planes)"""
        L, d, bias = lib(), C.byref(plan.desc), ctx.bias
        act = ctx.act if use_act else ACT_NONE
        if head is None:
            _ck(L.muvo_conv_prepare_dy(d, _f(y) if use_act else None, _f(dy), act, _fl(ctx.slope), _p(planes),
                                       _f(grad_of(bias)) if bias is not None else None, _st()))
            return dy, planes
        gl, head_w, head_b, head_wgrad = head
        co = head_w.shape[0]
        # with an activation the pass reads y anyway: the head's weight / bias gradient rides along
        ride = use_act and head_w.requires_grad
        if not ride:
            head_wgrad()
        _ck(L.muvo_conv_prepare_dy_head(d, _f(y) if use_act else None, _f(dy) if dy is not None else None,
                                        _f(gl.contiguous()), _f(head_w.contiguous().view(co, -1)), co, act, _fl(ctx.slope),
                                        _p(planes), _f(grad_of(bias)) if bias is not None else None,
                                        _f(grad_of(head_w)) if ride else None,
                                        _f(grad_of(head_b)) if (ride and head_b is not None) else None, _st()))
        if dy is None:
            dy = y if y is not None else x     # placeholder pointer: the bf16x3 kernels read the planes only
        return dy, planes

    @staticmethod
    def _data_grad(ctx, plan, x, dz, planes, fused_dy, dy_ws):
        """-> (dx, the dy workspace the kernel used: the given planes, or where it split dz itself; None if it needs none)"""
        wp = _packed_weight(plan, ctx.packed, ctx.weight, 1)
        dx = torch.empty(x.shape, device=dz.device, dtype=torch.float32)
        e1 = _bracket(plan, 'dgrad') if KERNEL_TIMING is not None else None
        if planes is None and (plan.ws_dgrad_dy > 0 or plan.ws_wgrad_dy > 0):
            planes = dy_ws.get(plan.dy_planes_floats)
        _ck(lib().muvo_conv_dgrad(C.byref(plan.desc), _f(dz), _f(wp), _f(dx), _p(planes), 1 if fused_dy else 0, _st()))
        if e1 is not None:
            e1.record()
        return dx, planes

    @staticmethod
    def _weight_grad(ctx, plan, x, y, dz, ws_dy, dy_is_split, fused_dy, dy_ws):
        """dy_is_split: ws_dy already holds the split planes of dz"""
        bias = ctx.bias
        gw = grad_of(ctx.weight)
        db = grad_of(bias) if (bias is not None and not fused_dy) else None   # fused_dy: already accumulated
        ws_x = ctx.ws_x
        x_ph = getattr(ctx, 'x_is_placeholder', False)
        xptr = ws_x if x_ph else x            # a planes-only input has no fp32 storage: the kernels read ctx.ws_x (flags bit 0)
        flags = (1 if ws_x is not None else 0) | (2 if (dy_is_split and plan.ws_wgrad_dy > 0) else 0)
        with _on_wgrad_stream(dy_ws.wst, x.device, (xptr, y, dz, ws_x, ctx.aff), dy_ws.slot):
            ws = scratch_zeroed('wgrad', plan.pack_fwd, x.device)         # (per stream)
            e1 = _bracket(plan, 'wgrad') if KERNEL_TIMING is not None else None
            if ws_x is None and plan.ws_wgrad_x:
                ws_x = scratch('conv_ws', (plan.ws_wgrad_x + 3) // 4, x.device)
            if plan.ws_wgrad_dy and ws_dy is None:
                ws_dy = scratch('conv_ws_dy', (plan.ws_wgrad_dy + 3) // 4, x.device)
            if ctx.aff is not None:
                _ck(lib().muvo_conv_wgrad_affine(C.byref(plan.desc), _f(x), _f(ctx.aff), _f(dz), _f(gw), _f(db), _st()))
            else:
                assert not x_ph or (flags & 1)
                _ck(lib().muvo_conv_wgrad(C.byref(plan.desc), _f(xptr), _f(dz), _f(ws), _f(gw), _f(db), _p(ws_x), _p(ws_dy),
                                          flags, _st()))
            if e1 is not None:
                e1.record()


def conv(x, weight, bias, geom, packed, act=ACT_NONE, slope=0.0, act_bwd_fused=False, moments=None, lazy=None):
    """lazy: (raw, aff) of a lazy AdaIN whose placeholder output is x (adain_lazy); the convolution applies the AdaIN itself."""
    if lazy is not None:
        return ConvFn.apply(x, weight, bias, geom, packed, act, slope, act_bwd_fused, moments, lazy[0], lazy[1])
    y = ConvFn.apply(x, weight, bias, geom, packed, act, slope, act_bwd_fused, moments)
    if (BN_PLANES and bias is None and act == ACT_NONE and moments is None and x.requires_grad and weight.requires_grad
            and torch.is_grad_enabled() and geom.plan_for(x).dy_planes):
        # the backward of this convolution reads dy as split planes (ConvFn._backward: fused_dy): a BatchNorm behind it may hand
        # its dx over in that form (bn_act(from_conv=True))
        y._muvo_dy_planes_ok = True
    return y


CONV_AFFINE = os.environ.get('MUVO_CONV_AFFINE', '1') != '0'


def conv_affine_supported(x, geom, moments):
    """can the convolution `geom` consume x = the (not yet normalised) output of the previous layer together with that layer's
    AdaIN as a per-(n, channel) scale / shift (muvo_conv_forward_affine)?  Needs the statistics from the producer's epilogue."""
    if not CONV_AFFINE or moments is None or x.dim() != 5 or not (x.requires_grad and torch.is_grad_enabled()):
        return False
    return geom.plan_for(x).supports('muvo_conv_affine_supported')


CONV_MOMENTS = os.environ.get('MUVO_CONV_MOMENTS', '1') != '0'


def conv_moments_buffer(x, geom):
    """A zeroed (N, Cout, 2) float64 buffer if the convolution `geom` on input x can deliver the instance-norm statistics of
    its output from its epilogue (muvo_conv_forward_moments), else None.  The buffer is per layer and stays all-zero between
    uses (muvo_adain_fwd_moments clears it)."""
    if not CONV_MOMENTS or not geom.plan_for(x).supports('muvo_conv_forward_moments_supported'):
        return None
    n = x.shape[0]
    cache = geom.__dict__.setdefault('_moments', {})       # one zeroed buffer per batch size (training / validation / imagination)
    buf = cache.get((n, x.device))
    if buf is None:
        buf = cache[(n, x.device)] = torch.zeros(n, geom.cout, 2, device=x.device, dtype=torch.float64)
        _MOMENT_BUFS.append(weakref.ref(buf))
    return buf


def _grad_is_private(g):
    """May a backward function write into the gradient tensor it was handed?  Only if nobody else holds it: autograd hands the SAME
    tensor to several consumers when a gradient is shared (both inputs of an add, expand views, retained grads / hooks).  Inside
    backward() a tensor made for this one consumer has two owners (the engine's input buffer and the Python argument); a shared
    one has more, or is a view (tests/test_kernels_gpu.py::test_head_branch_shared_gradient)."""
    return g._base is None and g._use_count() <= 2


class HeadBranchFn(torch.autograd.Function):
    """x -> (x, head(x)) for a 1x1 output head that hangs off a decoder trunk (ConvDecoder / VoxelDecoder1: head_4 and head_2
    read the feature map that also feeds the next stage, common.py:520-545,608-632).  Forward is the plain head convolution.
    Backward: the trunk's gradient arrives as the gradient of the first output; the head's data gradient is ACCUMULATED into
    that tensor by the kernel (muvo_conv_dgrad_accumulate) instead of autograd adding two full feature maps in a separate
    pass (3 x 681 MB at the rgb 1/2-scale level)."""

    @staticmethod
    def forward(ctx, x, weight, bias, geom, packed):
        y = ConvFn.forward(ctx, x, weight, bias, geom, packed, ACT_NONE, 0.0)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, gx, gy):
        x, _ = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        if gy is None:
            return (gx,) + (None,) * 4
        plan = ctx.geom.plan_for(x)
        L, d = lib(), C.byref(plan.desc)
        gy = gy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            wp = _packed_weight(plan, ctx.packed, weight, 1)
            if gx is not None and gx.is_contiguous() and _grad_is_private(gx):
                dx = gx            # a fresh tensor made by the trunk's backward for this one consumer: accumulated in place
                _ck(L.muvo_conv_dgrad_accumulate(d, _f(gy), _f(wp), _f(dx), _st()))
            else:
                dx = torch.empty_like(x)
                _ck(L.muvo_conv_dgrad(d, _f(gy), _f(wp), _f(dx), None, 0, _st()))
                if gx is not None:
                    dx = dx + gx
        if weight.requires_grad:
            ws = scratch_zeroed('wgrad', plan.pack_fwd, x.device)
            _ck(L.muvo_conv_wgrad(d, _f(x), _f(gy), _f(ws), _f(grad_of(weight)), _f(grad_of(bias)) if bias is not None else None,
                                  None, None, 0, _st()))
        return (dx,) + (None,) * 4


class ConvHeadFn(torch.autograd.Function):
    """(y, logits) = (act(conv(x)), head(y)) for a decoder stage whose output feeds a 1x1 head with <= 4 produced channels
    (ConvDecoder: trans_conv1/2/3 + head_4/2/1, common.py:608-632).  Forward: the two convolutions.  Backward: the head's weight /
    bias gradient, then the stage's own backward with the head's data gradient added to dy INSIDE the split pass
    (muvo_conv_prepare_dy_head) — neither the accumulate pass over the feature map (HeadBranchFn) nor, at the last stage, the
    materialised head gradient exists."""

    @staticmethod
    def forward(ctx, x, weight, bias, geom, packed, act, slope, head_w, head_b, head_geom, head_packed):
        plan = geom.plan_for(x)
        co = head_geom.cout
        fused = plan.supports('muvo_conv_forward_head_supported', co)
        logits = None
        if fused:
            # the head's forward rides on the stage's epilogue (muvo_conv_forward_head): no pass over y
            logits = torch.empty((plan.n, co) + plan.oshape[2:], device=x.device, dtype=torch.float32)
            ctx._head_fwd = (head_w.contiguous().view(co, -1), head_b, logits)
        y = ConvFn.forward(ctx, x, weight, bias, geom, packed, act, slope)
        ctx._head_fwd = None
        ctx.save_for_backward(x, y)            # y is needed for the head's weight gradient even when act needs no derivative
        ctx.head = (head_w, head_b, head_geom)
        # an output nobody differentiates through (the last stage's feature map has the head as its only consumer) arrives
        # as None in backward instead of a zero tensor of its size (1.36 GB filled, then read by the split pass)
        ctx.set_materialize_grads(False)
        if not fused:
            hplan = head_geom.plan_for(y)
            hwp = _packed_weight(hplan, head_packed, head_w, 0)
            logits = torch.empty(hplan.oshape, device=x.device, dtype=torch.float32)
            _ck(lib().muvo_conv_forward(C.byref(hplan.desc), _f(y), _f(hwp), _f(head_b), _f(logits), ACT_NONE, _fl(0.0), None, _st()))
        return y, logits

    @staticmethod
    def backward(ctx, gy, gl):
        if gl is None:
            if gy is None:
                return (None,) * 11
            return ConvFn._backward(ctx, gy, None)[:7] + (None,) * 4
        x, y = ctx.saved_tensors
        head_w, head_b, head_geom = ctx.head
        hplan = head_geom.plan_for(y)
        gl = gl.contiguous()

        def head_wgrad():        # the head's own weight-gradient pass (when it cannot ride on the split pass)
            if head_w.requires_grad:
                ws = scratch_zeroed('wgrad', hplan.pack_fwd, x.device)
                _ck(lib().muvo_conv_wgrad(C.byref(hplan.desc), _f(y), _f(gl), _f(ws), _f(grad_of(head_w)),
                                          _f(grad_of(head_b)) if head_b is not None else None, None, None, 0, _st()))
        return ConvFn._backward(ctx, gy, (gl, head_w, head_b, head_wgrad))[:7] + (None,) * 4


def conv_head_supported(x, geom, head_geom, act_bwd_fused=False):
    """can (stage convolution, 1x1 head) run as ConvHeadFn?  The head must be on the 1x1 head kernels, the stage on the bf16x3
    kernels in both gradient directions (its backward preamble is the split pass that absorbs the head's data gradient)."""
    if not CONV_HEAD or not (x.requires_grad and torch.is_grad_enabled()) or act_bwd_fused:
        return False
    plan = geom.plan_for(x)
    if not (plan.fam_dgrad == 1 and plan.fam_wgrad == 1):
        return False
    hplan = head_geom.plan(plan.n, plan.out_sz)
    return (hplan.fam_fwd == 3 and hplan.fam_wgrad == 3
            and plan.supports('muvo_conv_prepare_dy_head_supported', head_geom.cout))


CONV_HEAD = os.environ.get('MUVO_CONV_HEAD', '1') != '0'


def conv_head(x, weight, bias, geom, packed, act, slope, head_w, head_b, head_geom, head_packed):
    return ConvHeadFn.apply(x, weight, bias, geom, packed, act, slope, head_w, head_b, head_geom, head_packed)


def head_branch(x, weight, bias, geom, packed):
    """(x, head(x)); fused backward when the head runs on the 1x1 head kernels, plain conv otherwise."""
    plan = geom.plan_for(x)
    if plan.fam_fwd == 3 and plan.fam_dgrad == 3 and plan.fam_wgrad == 3 and x.requires_grad and torch.is_grad_enabled():
        return HeadBranchFn.apply(x, weight, bias, geom, packed)
    return x, conv(x, weight, bias, geom, packed)


# ================================================================================================ norms
BN_PLANES = os.environ.get('MUVO_BN_PLANES', '1') != '0'


_NAN_SCALAR = {}


def _nan_placeholder(shape, device):
    """a tensor of `shape` without storage of its size (one NaN, expanded): stands for data that exists only as split planes
    (attribute _muvo_planes).  Anything that reads it as numbers gets NaN - a misuse cannot go unnoticed.  The one-element source
    is made once per device (a fresh torch.full per call was 60 fill launches per step); every call returns a new view object, so
    attributes set on one placeholder do not show up on another."""
    device = torch.device(device)
    src = _NAN_SCALAR.get(device)
    if src is None:
        src = _NAN_SCALAR[device] = torch.full((1,), float('nan'), device=device, dtype=torch.float32)
    return src.expand(shape)


class BNActFn(torch.autograd.Function):
    """Train-mode BatchNorm2d + optional residual + ReLU.  res_mode 1: relu(bn(x)+res); 2: relu(bn(x))+res.
    planes: also write the channels-last bf16 hi / lo planes of the result (what a bf16x3 convolution reads;
    muvo_bn_train_fwd_planes) and hand them to the consumers as y._muvo_planes; keep_f32=False: ONLY the planes (y is a
    NaN placeholder) - the caller guarantees that the sole consumer is a convolution that reads planes in forward and weight
    gradient.  dx_planes: the input x is the output of a convolution whose backward reads split planes of its dy
    (x._muvo_dy_planes_ok): backward writes dx as planes only (muvo_bn_train_bwd_planes)."""

    @staticmethod
    def forward(ctx, x, residual, bn, res_mode, relu, training, planes=False, keep_f32=True, dx_planes=False):
        x = x.contiguous()
        n, c = x.shape[:2]
        s = x.numel() // (n * c)
        mean = torch.empty(c, device=x.device, dtype=torch.float32)
        rstd = torch.empty(c, device=x.device, dtype=torch.float32)
        if residual is not None:
            residual = residual.contiguous()
        if not training:
            raise RuntimeError('eval-mode BatchNorm is not part of the training hot path (reference keeps train() mode '
                               'even in validation, trainer.py:405)')
        mask_mode = 0 if not relu else (1 if (residual is not None and res_mode == 1) else 2)
        keep_f32 = keep_f32 or not planes or mask_mode == 1
        y = torch.empty_like(x) if keep_f32 else _nan_placeholder(x.shape, x.device)
        if planes:
            pl = torch.empty((lib().muvo_split_planes_bytes(n, c, _i64(s)) + 3) // 4, device=x.device, dtype=torch.float32)
            _ck(lib().muvo_bn_train_fwd_planes(_f(x), _f(bn.weight), _f(bn.bias), _f(residual), _f(y) if keep_f32 else None, _f(mean),
                                               _f(rstd), _f(bn.running_mean), _f(bn.running_var), n, c, _i64(s), _fl(bn.eps),
                                               _fl(bn.momentum), res_mode if residual is not None else 0, int(relu), _p(pl), _st()))
            _BN_PLANES_OUT.append((pl, _stream_key(x.device), not keep_f32))
        else:
            ws = torch.empty(2 * c, device=x.device, dtype=torch.float64)
            _ck(lib().muvo_bn_train_fwd(_f(x), _f(bn.weight), _f(bn.bias), _f(residual), _f(y), _f(mean), _f(rstd),
                                        _f(bn.running_mean), _f(bn.running_var), _p(ws), n, c, _i64(s), _fl(bn.eps),
                                        _fl(bn.momentum), res_mode if residual is not None else 0, int(relu), _st()))
        _BN_PENDING.append(bn)           # num_batches_tracked += 1, applied in one fused launch (flush_bn_counters)
        ctx.bn, ctx.dims = bn, (n, c, s)
        # ReLU mask in backward: recomputed from x (mode 2: y is neither saved nor re-read) unless the ReLU sits AFTER the
        # residual add (res_mode 1), where only y knows the sign
        ctx.mask_mode = mask_mode
        ctx.has_res, ctx.res_mode = residual is not None, res_mode
        ctx.dx_planes = bool(dx_planes)
        ctx.save_for_backward(x, y if ctx.mask_mode == 1 else None, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, rstd = ctx.saved_tensors
        bn = ctx.bn
        n, c, s = ctx.dims
        dy = dy.contiguous()
        dres = None
        if ctx.has_res and ctx.needs_input_grad[1]:
            dres = torch.empty_like(x) if ctx.res_mode == 1 else dy
        if ctx.dx_planes:
            # dx leaves as the split planes the producing convolution's data- and weight-gradient kernels read; no fp32 dx
            pl = torch.empty((lib().muvo_split_planes_bytes(n, c, _i64(s)) + 3) // 4, device=x.device, dtype=torch.float32)
            _ck(lib().muvo_bn_train_bwd_planes(_f(x), _f(y), _f(dy), _f(bn.weight), _f(bn.bias), _f(mean), _f(rstd), None,
                                               _f(dres) if (ctx.has_res and ctx.res_mode == 1) else None,
                                               _f(grad_of(bn.weight)), _f(grad_of(bn.bias)), n, c, _i64(s), ctx.mask_mode, _p(pl), _st()))
            dx = _nan_placeholder(x.shape, x.device)
            dx._muvo_planes = (pl, _stream_key(x.device))
            return dx, dres, None, None, None, None, None, None, None
        dx = torch.empty_like(x)
        ws = torch.empty(2 * c, device=x.device, dtype=torch.float64)
        _ck(lib().muvo_bn_train_bwd(_f(x), _f(y), _f(dy), _f(bn.weight), _f(bn.bias), _f(mean), _f(rstd), _f(dx),
                                    _f(dres) if (ctx.has_res and ctx.res_mode == 1) else None,
                                    _f(grad_of(bn.weight)), _f(grad_of(bn.bias)), _p(ws), n, c, _i64(s), ctx.mask_mode,
                                    _st()))
        return dx, dres, None, None, None, None, None, None, None


_BN_PENDING = []


def flush_bn_counters():
    """Apply the pending `num_batches_tracked += 1` of every BatchNorm forward since the last flush with one
    torch._foreach_add_ (76 one-element launches per step otherwise).  Called at the start of every training forward and
    before a BatchNorm's buffers are read (state_dict)."""
    if not _BN_PENDING:
        return
    counts = {}
    for bn in _BN_PENDING:
        counts[id(bn)] = (bn, counts.get(id(bn), (bn, 0))[1] + 1)
    _BN_PENDING.clear()
    by_k = {}
    for bn, k in counts.values():
        by_k.setdefault(k, []).append(bn.num_batches_tracked)
    for k, tensors in by_k.items():
        torch._foreach_add_(tensors, k)


def conv_reads_planes(conv, x_shape, need_wgrad):
    """will the convolution module `conv` read split planes of an input of shape x_shape in forward (and, if a backward follows,
    in its weight gradient)?  -> (forward reads planes, and the fp32 values are needed by nobody inside the convolution)"""
    plan = conv.geom.plan_for(x_shape)
    fwd = plan.fam_fwd == 1 and plan.ws_fwd_x > 0
    return fwd, fwd and (not need_wgrad or (plan.fam_wgrad == 1 and plan.ws_wgrad_x > 0 and _KEEP_WS))


def bn_act(x, bn, residual=None, res_mode=1, relu=True, consumers=(), sole_consumer=False, from_conv=False):
    """consumers: convolution modules that will read the result (planes are written with it when at least one of them runs on the
    bf16x3 kernels); sole_consumer: `consumers` is everything that reads the result, so the fp32 tensor is dropped when they all
    read planes; from_conv: x is the output of a bias-free convolution without activation and this BatchNorm is its only
    consumer (conv -> bn): dx is handed to that convolution's backward as planes when it reads planes."""
    planes, keep_f32 = False, True
    if BN_PLANES and consumers and x.is_cuda:
        grad = torch.is_grad_enabled() and x.requires_grad
        rd = [conv_reads_planes(cv, x.shape, grad and cv.weight.requires_grad) for cv in consumers]
        planes = any(r[0] for r in rd)
        keep_f32 = not (sole_consumer and all(r[1] for r in rd))
    dx_planes = BN_PLANES and from_conv and getattr(x, '_muvo_dy_planes_ok', False)
    y = BNActFn.apply(x, residual, bn, res_mode, relu, bn.training, planes, keep_f32, dx_planes)
    if planes:
        pl = _BN_PLANES_OUT.pop()
        y._muvo_planes = pl[:2]
        if pl[2]:
            y._muvo_planes_only = True
    return y


_BN_PLANES_OUT = []


class AdaINFn(torch.autograd.Function):
    """AdaptiveInstanceNorm3d. x: (N,C,D,H,W) or a broadcast (C,D,H,W) parameter; style: (N, 2C)."""

    @staticmethod
    def forward(ctx, x, style, eps, n_batch, pre_act=ACT_NONE, pre_slope=0.0, moments=None, aff_out=None):
        x = x.contiguous()
        style = style.contiguous()
        bcast = x.dim() == 4
        ctx.pre_act, ctx.pre_slope = pre_act, pre_slope
        c = x.shape[0] if bcast else x.shape[1]
        s = x.numel() // c if bcast else x.numel() // (x.shape[0] * c)
        n = n_batch
        mean = torch.empty(n * c, device=x.device, dtype=torch.float32)
        rstd = torch.empty(n * c, device=x.device, dtype=torch.float32)
        if aff_out is not None:
            # lazy form: statistics -> (mean, rstd, scale / shift table); the consumer applies the map while staging x, the
            # normalised tensor is never written.  The returned tensor is a shape-only placeholder (no storage of its size).
            _ck(lib().muvo_adain_affine(_f(style), _p(moments), _f(mean), _f(rstd), _f(aff_out), n, c, _i64(s), _fl(eps), _st()))
            ctx.dims = (n, c, s, bcast)
            ctx.save_for_backward(x, style, mean, rstd)
            return torch.empty(1, device=x.device, dtype=torch.float32).expand((n, c) + tuple(x.shape[-3:]))
        y = torch.empty((n, c) + tuple(x.shape[-3:]), device=x.device, dtype=torch.float32)
        if moments is not None and not bcast:   # statistics already accumulated by the producing convolution's epilogue
            _ck(lib().muvo_adain_fwd_moments(_f(x), _f(style), _f(y), _f(mean), _f(rstd), _p(moments), n, c, _i64(s), _fl(eps), _st()))
        else:
            ws = torch.empty(2 * n * c, device=x.device, dtype=torch.float64)
            _ck(lib().muvo_adain_fwd(_f(x), _f(style), _f(y), _f(mean), _f(rstd), _p(ws), n, c, _i64(s),
                                     _i64(0 if bcast else c * s), _fl(eps), _st()))
        ctx.dims = (n, c, s, bcast)
        ctx.save_for_backward(x, style, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, style, mean, rstd = ctx.saved_tensors
        n, c, s, bcast = ctx.dims
        dy = dy.contiguous()
        dxf = torch.empty_like(dy)
        dstyle = torch.empty_like(style)
        ws = torch.empty(2 * n * c, device=x.device, dtype=torch.float64)
        _ck(lib().muvo_adain_bwd(_f(x), _f(style), _f(dy), _f(mean), _f(rstd), _f(dxf), _f(dstyle), _p(ws), n, c,
                                 _i64(s), _i64(0 if bcast else c * s), ctx.pre_act, _fl(ctx.pre_slope), _st()))
        if bcast:
            dx = torch.empty_like(x)
            _ck(lib().muvo_batchsum(_f(dxf), _f(dx), n, _i64(c * s), 0, _st()))
        else:
            dx = dxf
        return dx, dstyle, None, None, None, None, None, None


def adain_lazy(x, style, eps, pre_act, pre_slope, moments):
    """AdaIN of x (N, C, D, H, W) whose consumer applies it while staging: returns (placeholder, x, aff) for
    conv(..., lazy=(x, aff)).  The placeholder carries the autograd edge and the shape, nothing else may read it."""
    n, c = x.shape[:2]
    aff = torch.empty(n, c, 2, device=x.device, dtype=torch.float32)
    y = AdaINFn.apply(x, style, eps, n, pre_act, pre_slope, moments, aff)
    return y, x, aff


def adain(x, style, eps, n_batch, pre_act=ACT_NONE, pre_slope=0.0, moments=None):
    """pre_act: x is the output of that activation and the producer's backward does NOT apply its derivative (the
    AdaIN backward kernel chains it); pair with conv(..., act_bwd_fused=True)."""
    return AdaINFn.apply(x, style, eps, n_batch, pre_act, pre_slope, moments)


class AdaINHeadFn(torch.autograd.Function):
    """AdaIN of the last voxel-decoder convolution + the 1x1x1 class head in one pass each way (csrc/norm.hip:
    adain_head_*): x (N,C,D,H,W) is the convolution output (LeakyReLU applied, its derivative chained here), `moments` its
    per-(n,c) sums from the convolution epilogue.  The normalised tensor never exists in HBM."""

    @staticmethod
    def forward(ctx, x, style, head_w, head_b, eps, moments, pre_act, pre_slope):
        x, style = x.contiguous(), style.contiguous()
        n, c = x.shape[:2]
        s = x.numel() // (n * c)
        co = head_w.shape[0]
        logits = torch.empty((n, co) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
        mean = torch.empty(n * c, device=x.device, dtype=torch.float32)
        rstd = torch.empty(n * c, device=x.device, dtype=torch.float32)
        _ck(lib().muvo_adain_head_fwd(_f(x), _f(style), _f(mean), _f(rstd), _p(moments), _f(head_w.contiguous().view(co, c)),
                                      _f(head_b), _f(logits), n, c, co, _i64(s), _fl(eps), _st()))
        ctx.dims, ctx.pre = (n, c, co, s), (pre_act, pre_slope)
        ctx.head_w, ctx.head_b = head_w, head_b
        ctx.save_for_backward(x, style, mean, rstd)
        return logits

    @staticmethod
    def backward(ctx, dl):
        x, style, mean, rstd = ctx.saved_tensors
        n, c, co, s = ctx.dims
        head_w, head_b = ctx.head_w, ctx.head_b
        dl = dl.contiguous()
        dx = torch.empty_like(x)
        dstyle = torch.empty_like(style)
        ws = torch.empty(2 * n * c, device=x.device, dtype=torch.float64)
        _ck(lib().muvo_adain_head_bwd(_f(x), _f(style), _f(mean), _f(rstd), _f(head_w.contiguous().view(co, c)), _f(dl), _f(dx),
                                      _f(dstyle), _f(grad_of(head_w)), _f(grad_of(head_b)) if head_b is not None else None, _p(ws),
                                      n, c, co, _i64(s), ctx.pre[0], _fl(ctx.pre[1]), _st()))
        return dx, dstyle, None, None, None, None, None, None


ADAIN_HEAD = os.environ.get('MUVO_ADAIN_HEAD', '1') != '0'


def adain_head_supported(x, head_w, moments):
    if not ADAIN_HEAD or moments is None or x.dim() != 5:
        return False
    n, c = x.shape[:2]
    return bool(lib().muvo_adain_head_supported(c, head_w.shape[0], _i64(x.numel() // (n * c)))) and n <= 65535


def adain_head(x, style, head_w, head_b, eps, moments, pre_act=ACT_NONE, pre_slope=0.0):
    return AdaINHeadFn.apply(x, style, head_w, head_b, eps, moments, pre_act, pre_slope)


class AddDropoutLNFn(torch.autograd.Function):
    """y = LayerNorm(x + dropout(a)) over the last dim."""

    @staticmethod
    def forward(ctx, x, a, ln, p, seed):
        x = x.contiguous()
        a = a.contiguous()
        e = x.shape[-1]
        rows = x.numel() // e
        y = torch.empty_like(x)
        z = torch.empty_like(x)
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
        _ck(lib().muvo_add_dropout_layernorm_fwd(_f(x), _f(a), _f(ln.weight), _f(ln.bias), _f(y), _f(z), _f(mean),
                                                 _f(rstd), rows, e, _fl(ln.eps), _fl(p), C.c_uint64(seed), _st()))
        ctx.ln, ctx.p, ctx.seed, ctx.dims = ln, p, seed, (rows, e)
        ctx.save_for_backward(z, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, mean, rstd = ctx.saved_tensors
        ln = ctx.ln
        rows, e = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        da = torch.empty_like(dy)
        _ck(lib().muvo_add_dropout_layernorm_bwd(_f(dy), _f(z), _f(mean), _f(rstd), _f(ln.weight), _f(dx), _f(da),
                                                 _f(grad_of(ln.weight)), _f(grad_of(ln.bias)), rows, e, _fl(ctx.p),
                                                 C.c_uint64(ctx.seed), _st()))
        return dx, da, None, None, None


def add_dropout_layernorm(x, a, ln, p, seed):
    return AddDropoutLNFn.apply(x, a, ln, p, seed)


# ================================================================================================ misc
class ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, slope):
        x = x.contiguous()
        y = torch.empty_like(x)
        _ck(lib().muvo_act_fwd(_f(x), _f(y), _i64(x.numel()), act, _fl(slope), _st()))
        ctx.act, ctx.slope = act, slope
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        _ck(lib().muvo_act_bwd(_f(y), _f(dy), _f(dx), _i64(dy.numel()), ctx.act, _fl(ctx.slope), _st()))
        return dx, None, None


def activation(x, act, slope=0.0):
    return ActFn.apply(x, act, slope)


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        x = x.contiguous()
        y = torch.empty_like(x)
        _ck(lib().muvo_dropout(_f(x), _f(y), _i64(x.numel()), _fl(p), C.c_uint64(seed), _st()))
        ctx.p, ctx.seed = p, seed
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        _ck(lib().muvo_dropout(_f(dy), _f(dx), _i64(dy.numel()), _fl(ctx.p), C.c_uint64(ctx.seed), _st()))
        return dx, None, None


def dropout(x, p, seed):
    if p <= 0.0:
        return x
    return DropoutFn.apply(x, p, seed)


class CatLastFn(torch.autograd.Function):
    """torch.cat(tensors, dim=-1) for 2-D row-major tensors, via strided 2-D copies."""

    @staticmethod
    def forward(ctx, *xs):
        rows = xs[0].shape[0]
        widths = [x.shape[1] for x in xs]
        tot = sum(widths)
        y = torch.empty(rows, tot, device=xs[0].device, dtype=torch.float32)
        off = 0
        for x, w in zip(xs, widths):
            x = x.contiguous()
            _ck(lib().muvo_copy2d(_f(x), C.c_void_p(y.data_ptr() + 4 * off), _i64(rows), _i64(w), _i64(w), _i64(tot), 0,
                                  _st()))
            off += w
        ctx.widths, ctx.rows = widths, rows
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        tot = sum(ctx.widths)
        outs, off = [], 0
        for i, w in enumerate(ctx.widths):
            if ctx.needs_input_grad[i]:
                g = torch.empty(ctx.rows, w, device=dy.device, dtype=torch.float32)
                _ck(lib().muvo_copy2d(C.c_void_p(dy.data_ptr() + 4 * off), _f(g), _i64(ctx.rows), _i64(w), _i64(tot),
                                      _i64(w), 0, _st()))
                outs.append(g)
            else:
                outs.append(None)
            off += w
        return tuple(outs)


def cat_last(xs):
    return CatLastFn.apply(*xs)


class SliceLastFn(torch.autograd.Function):
    """x[:, a:b] as a fresh contiguous tensor (2-D)."""

    @staticmethod
    def forward(ctx, x, a, b):
        x = x.contiguous()
        rows, tot = x.shape
        y = torch.empty(rows, b - a, device=x.device, dtype=torch.float32)
        _ck(lib().muvo_copy2d(C.c_void_p(x.data_ptr() + 4 * a), _f(y), _i64(rows), _i64(b - a), _i64(tot), _i64(b - a), 0,
                              _st()))
        ctx.a, ctx.b, ctx.tot, ctx.rows = a, b, tot, rows
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.zeros(ctx.rows, ctx.tot, device=dy.device, dtype=torch.float32)
        _ck(lib().muvo_copy2d(_f(dy), C.c_void_p(dx.data_ptr() + 4 * ctx.a), _i64(ctx.rows), _i64(ctx.b - ctx.a),
                              _i64(ctx.b - ctx.a), _i64(ctx.tot), 0, _st()))
        return dx, None, None


def slice_last(x, a, b):
    return SliceLastFn.apply(x, a, b)


class TokensFn(torch.autograd.Function):
    """(N,C,h,w) feature maps of the two sensors -> (L_img+L_lidar, N, C) tokens with positional + type embedding."""

    @staticmethod
    def forward(ctx, xi, xl, pos_i, pos_l, type_emb):
        xi, xl = xi.contiguous(), xl.contiguous()
        n, c = xi.shape[:2]
        li, ll = xi.shape[2] * xi.shape[3], xl.shape[2] * xl.shape[3]
        tok = torch.empty(li + ll, n, c, device=xi.device, dtype=torch.float32)
        L = lib()
        te = type_emb.contiguous()  # (1,1,C,2): element [c][k] at c*2+k
        _ck(L.muvo_nchw_to_tokens(_f(xi), _f(pos_i), _f(te), 2, _f(tok), n, c, li, 0, _st()))
        _ck(L.muvo_nchw_to_tokens(_f(xl), _f(pos_l), C.c_void_p(te.data_ptr() + 4), 2, _f(tok), n, c, ll, li, _st()))
        ctx.shapes = (xi.shape, xl.shape, li, ll, n, c)
        ctx.type_emb = type_emb
        return tok

    @staticmethod
    def backward(ctx, dtok):
        dtok = dtok.contiguous()
        si, sl, li, ll, n, c = ctx.shapes
        L = lib()
        dxi = torch.empty(si, device=dtok.device, dtype=torch.float32)
        dxl = torch.empty(sl, device=dtok.device, dtype=torch.float32)
        _ck(L.muvo_tokens_to_nchw(_f(dtok), _f(dxi), n, c, li, 0, _st()))
        _ck(L.muvo_tokens_to_nchw(_f(dtok), _f(dxl), n, c, ll, li, _st()))
        te = ctx.type_emb
        if te.requires_grad:
            tmp = torch.zeros(2, c, device=dtok.device, dtype=torch.float32)
            _ck(L.muvo_colsum_acc(_f(dtok), _f(tmp[0]), _i64(li * n), _i64(c), _i64(c), _st()))
            _ck(L.muvo_colsum_acc(C.c_void_p(dtok.data_ptr() + 4 * li * n * c), _f(tmp[1]), _i64(ll * n), _i64(c),
                                  _i64(c), _st()))
            # grad layout (1,1,C,2): interleave the two columns with strided copies
            g = grad_of(te)
            for k in range(2):
                _ck(L.muvo_copy2d(_f(tmp[k]), C.c_void_p(g.data_ptr() + 4 * k), _i64(c), _i64(1), _i64(1), _i64(2), 1,
                                  _st()))
        return dxi, dxl, None, None, None


def make_tokens(xi, xl, pos_i, pos_l, type_emb):
    return TokensFn.apply(xi, xl, pos_i, pos_l, type_emb)


class UntokenFn(torch.autograd.Function):
    """tokens[l0:l0+h*w] (L,N,C) -> (N,C,h,w)."""

    @staticmethod
    def forward(ctx, tok, l0, h, w):
        tok = tok.contiguous()
        ltot, n, c = tok.shape
        x = torch.empty(n, c, h, w, device=tok.device, dtype=torch.float32)
        _ck(lib().muvo_tokens_to_nchw(_f(tok), _f(x), n, c, h * w, l0, _st()))
        ctx.dims = (ltot, n, c, l0, h * w)
        return x

    @staticmethod
    def backward(ctx, dx):
        dx = dx.contiguous()
        ltot, n, c, l0, l = ctx.dims
        dtok = torch.zeros(ltot, n, c, device=dx.device, dtype=torch.float32)
        _ck(lib().muvo_nchw_to_tokens(_f(dx), None, None, 0, _f(dtok), n, c, l, l0, _st()))
        return dtok, None, None, None


def untoken(tok, l0, h, w):
    return UntokenFn.apply(tok, l0, h, w)


class MaxPool2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, p):
        x = x.contiguous()
        n, c, h, w = x.shape
        oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        y = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32)
        idx = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.uint8)
        _ck(lib().muvo_maxpool2d_fwd(_f(x), _f(y), _p(idx), _i64(n * c), h, w, oh, ow, k, s, p, _st()))
        ctx.dims = (n, c, h, w, oh, ow, k, s, p)
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        n, c, h, w, oh, ow, k, s, p = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty(n, c, h, w, device=dy.device, dtype=torch.float32)
        _ck(lib().muvo_maxpool2d_bwd(_f(dy), _p(idx), _f(dx), _i64(n * c), h, w, oh, ow, k, s, p, _st()))
        return dx, None, None, None


def max_pool2d(x, k, s=None, p=0):
    return MaxPool2dFn.apply(x, k, s or k, p)


class GlobalAvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        n, c = x.shape[:2]
        s = x.numel() // (n * c)
        y = torch.empty(n, c, device=x.device, dtype=torch.float32)
        _ck(lib().muvo_avgpool_fwd(_f(x), _f(y), _i64(n * c), _i64(s), _st()))
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        shape = ctx.shape
        dx = torch.empty(shape, device=dy.device, dtype=torch.float32)
        g = shape[0] * shape[1]
        _ck(lib().muvo_avgpool_bwd(_f(dy), _f(dx), _i64(g), _i64(dx.numel() // g), _st()))
        return dx


def global_avg_pool(x):
    return GlobalAvgPoolFn.apply(x)


class Upsample3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        n, c, d, h, w = x.shape
        y = torch.empty(n, c, 2 * d, 2 * h, 2 * w, device=x.device, dtype=torch.float32)
        _ck(lib().muvo_upsample3d_x2_fwd(_f(x), _f(y), _i64(n * c), d, h, w, _st()))
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        n, c, d, h, w = ctx.shape
        dx = torch.empty(ctx.shape, device=dy.device, dtype=torch.float32)
        _ck(lib().muvo_upsample3d_x2_bwd(_f(dy), _f(dx), _i64(n * c), d, h, w, _st()))
        return dx


def upsample3d_x2(x):
    return Upsample3dFn.apply(x)


UPSAMPLE_KERNELS = ('scalar', 'vec', 'row')


def upsample3d_route(backward, nc, d, h, w, in_addr=0, out_addr=0):
    """What upsample3d_x2 would launch forward (in / out = x / y) or backward (dy / dx), host code only, no device:
    dict(kernel, grid, block, segs, dseg).  The byte addresses count only by their 16-byte alignment."""
    r = Upsample3dRouteInfo()
    _ck(lib().muvo_upsample3d_route(int(bool(backward)), _i64(nc), d, h, w, C.c_void_p(in_addr), C.c_void_p(out_addr), C.byref(r)))
    return {'kernel': UPSAMPLE_KERNELS[r.kernel], 'grid': tuple(r.grid), 'block': tuple(r.block), 'segs': r.segs, 'dseg': r.dseg}


def maxpool2d_route(backward, nc, h, w, k, s, p, in_addr=0, idx_addr=0, out_addr=0):
    """What max_pool2d would launch forward (in / out = x / y) or backward (dy / dx), host code only, no device:
    dict(k, load16, v8, grid, block)."""
    r = MaxPool2dRouteInfo()
    _ck(lib().muvo_maxpool2d_route(int(bool(backward)), _i64(nc), h, w, k, s, p, C.c_void_p(in_addr), C.c_void_p(idx_addr),
                                   C.c_void_p(out_addr), C.byref(r)))
    return {'k': r.k, 'load16': bool(r.load16), 'v8': bool(r.v8), 'grid': tuple(r.grid), 'block': tuple(r.block)}


def softmax_dropout_route(cols):
    """The MAXV template instance (8 or 17) of the softmax(+dropout) kernels for rows of `cols` columns (host code only)."""
    r = lib().muvo_softmax_dropout_route(int(cols))
    if r < 0:
        _ck(r)
    return {'maxv': r}


# ================================================================================================ attention
class AttentionFn(torch.autograd.Function):
    """Multi-head self-attention core on a packed (L, N, 3E) qkv tensor -> (L, N, E).

    QK^T and PV are strided batched MFMA GEMMs straight on the packed layout (no head split copies);
    softmax + attention-probability dropout is one wave-per-row kernel."""

    @staticmethod
    def forward(ctx, qkv, nheads, p, seed):
        qkv = qkv.contiguous()
        l, n, e3 = qkv.shape
        e = e3 // 3
        dh = e // nheads
        scale = 1.0 / (dh ** 0.5)
        dev = qkv.device
        S = torch.empty(n, nheads, l, l, device=dev, dtype=torch.float32)
        # S[n][h][i][j] = scale * sum_d q[i][n][h*dh+d] * k[j][n][e + h*dh + d]
        gemm(qkv, qkv, S, l, l, dh, n * e3, 1, 1, n * e3, l, alpha=scale, B1=n, B2=nheads,
             a_b=(e3, dh), b_b=(e3, dh), c_b=(nheads * l * l, l * l), b_off=e)
        P = torch.empty_like(S)
        Pd = torch.empty_like(S) if p > 0 else None
        _ck(lib().muvo_softmax_dropout_fwd(_f(S), _f(P), _f(Pd), _i64(n * nheads * l), l, _fl(p), C.c_uint64(seed),
                                           _st()))
        del S
        o = torch.empty(l, n, e, device=dev, dtype=torch.float32)
        pa = Pd if Pd is not None else P
        # o[i][n][h*dh+d] = sum_j P[n][h][i][j] * v[j][n][2e + h*dh + d]
        gemm(pa, qkv, o, l, dh, l, l, 1, n * e3, 1, n * e, B1=n, B2=nheads, a_b=(nheads * l * l, l * l),
             b_b=(e3, dh), c_b=(e, dh), b_off=2 * e)
        ctx.dims = (l, n, e, nheads, dh, scale, p, seed)
        ctx.save_for_backward(qkv, P)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, P = ctx.saved_tensors
        l, n, e, nheads, dh, scale, p, seed = ctx.dims
        e3 = 3 * e
        do = do.contiguous()
        dev = do.device
        dqkv = torch.empty_like(qkv)
        if p > 0:
            Pd = torch.empty_like(P)
            _ck(lib().muvo_dropout(_f(P), _f(Pd), _i64(P.numel()), _fl(p), C.c_uint64(seed), _st()))
        else:
            Pd = P
        bP = (nheads * l * l, l * l)
        # dV[j][n][h*dh+d] = sum_i Pd[i][j] * do[i][n][h*dh+d]   (A(m=j,k=i)=Pd[i*l+j])
        gemm(Pd, do, dqkv, l, dh, l, 1, l, n * e, 1, n * e3, B1=n, B2=nheads, a_b=bP, b_b=(e, dh), c_b=(e3, dh),
             c_off=2 * e)
        # dPd[i][j] = sum_d do[i][n][h*dh+d] * v[j][n][2e+h*dh+d]
        dPd = torch.empty_like(P)
        gemm(do, qkv, dPd, l, l, dh, n * e, 1, 1, n * e3, l, B1=n, B2=nheads, a_b=(e, dh), b_b=(e3, dh), c_b=bP,
             b_off=2 * e)
        dS = dPd  # in place
        _ck(lib().muvo_softmax_dropout_bwd(_f(P), _f(dPd), _f(dS), _i64(n * nheads * l), l, _fl(p), C.c_uint64(seed),
                                           _st()))
        # dQ[i][.] = scale * sum_j dS[i][j] * k[j][.]
        gemm(dS, qkv, dqkv, l, dh, l, l, 1, n * e3, 1, n * e3, alpha=scale, B1=n, B2=nheads, a_b=bP, b_b=(e3, dh),
             c_b=(e3, dh), b_off=e)
        # dK[j][.] = scale * sum_i dS[i][j] * q[i][.]
        gemm(dS, qkv, dqkv, l, dh, l, 1, l, n * e3, 1, n * e3, alpha=scale, B1=n, B2=nheads, a_b=bP, b_b=(e3, dh),
             c_b=(e3, dh), c_off=e)
        return dqkv, None, None, None


class _FusedAttentionFn(torch.autograd.Function):
    """The same attention core as ONE kernel forward and two backward (csrc/attention.hip), no L x L tensor in HBM; saves qkv, o
    and the row log-sum-exp only, backward recomputes the probabilities from it.  The two paths of the unit subclass this with
    their entry points (FWD, BWD) and whether backward takes the D = do . o workspace, (N * heads, L) floats (DWS)."""
    FWD = BWD = None
    DWS = False

    @classmethod
    def forward(cls, ctx, qkv, nheads, p, seed):
        qkv = qkv.contiguous()
        l, n, e3 = qkv.shape
        e = e3 // 3
        o = torch.empty(l, n, e, device=qkv.device, dtype=torch.float32)
        lse = torch.empty(n * nheads, l, device=qkv.device, dtype=torch.float32)
        _ck(getattr(lib(), cls.FWD)(_f(qkv), _f(o), _f(lse), l, n, nheads, e // nheads, _fl(p), C.c_uint64(seed), _st()))
        ctx.dims = (l, n, nheads, e // nheads, p, seed)
        ctx.save_for_backward(qkv, o, lse)
        return o

    @classmethod
    def backward(cls, ctx, do):
        qkv, o, lse = ctx.saved_tensors
        l, n, nheads, dh, p, seed = ctx.dims
        dqkv = torch.empty_like(qkv)
        dws = torch.empty_like(lse) if cls.DWS else None
        _ck(getattr(lib(), cls.BWD)(_f(qkv), _f(o), _f(do.contiguous()), _f(lse), _f(dqkv), *((_f(dws),) if cls.DWS else ()), l, n,
                                    nheads, dh, _fl(p), C.c_uint64(seed), _st()))
        return dqkv, None, None, None


class FlashAttentionFn(_FusedAttentionFn):
    """Resident path (L <= 384): K / V of a head staged whole in LDS, softmax over register-resident score tiles with wave
    shuffles."""
    FWD, BWD = 'muvo_attention_fwd', 'muvo_attention_bwd'


class StreamAttentionFn(_FusedAttentionFn):
    """Streamed path, any sequence length: K / V pass through LDS block by block under an online softmax; the one extra buffer of
    backward is D."""
    FWD, BWD, DWS = 'muvo_attention_stream_fwd', 'muvo_attention_stream_bwd', True


class _MaskedAttentionFn(torch.autograd.Function):
    """_FusedAttentionFn with a key mask (N, L') uint8, rows padded to a multiple of 16 bytes (key_mask_rows), non-zero = the key
    is ignored; the semantics are in include/muvo_hip.h.  Backward saves the mask and returns None for it."""
    FWD = BWD = None
    DWS = False

    @classmethod
    def forward(cls, ctx, qkv, nheads, p, seed, mask):
        qkv = qkv.contiguous()
        l, n, e3 = qkv.shape
        e = e3 // 3
        o = torch.empty(l, n, e, device=qkv.device, dtype=torch.float32)
        lse = torch.empty(n * nheads, l, device=qkv.device, dtype=torch.float32)
        _ck(getattr(lib(), cls.FWD)(_f(qkv), _f(o), _f(lse), l, n, nheads, e // nheads, _fl(p), C.c_uint64(seed), _st(), _p(mask),
                                    _i64(mask.shape[1])))
        ctx.dims = (l, n, nheads, e // nheads, p, seed)
        ctx.save_for_backward(qkv, o, lse, mask)
        return o

    @classmethod
    def backward(cls, ctx, do):
        qkv, o, lse, mask = ctx.saved_tensors
        l, n, nheads, dh, p, seed = ctx.dims
        dqkv = torch.empty_like(qkv)
        dws = torch.empty_like(lse) if cls.DWS else None
        _ck(getattr(lib(), cls.BWD)(_f(qkv), _f(o), _f(do.contiguous()), _f(lse), _f(dqkv), *((_f(dws),) if cls.DWS else ()), l, n,
                                    nheads, dh, _fl(p), C.c_uint64(seed), _st(), _p(mask), _i64(mask.shape[1])))
        return dqkv, None, None, None, None


class MaskedFlashAttentionFn(_MaskedAttentionFn):
    FWD, BWD = 'muvo_attention_mask_fwd', 'muvo_attention_mask_bwd'


class MaskedStreamAttentionFn(_MaskedAttentionFn):
    FWD, BWD, DWS = 'muvo_attention_stream_mask_fwd', 'muvo_attention_stream_mask_bwd', True


FLASH_ATTENTION = os.environ.get('MUVO_FLASH_ATTN', '1') != '0'
# Shortest sequence the streamed kernels take from the unfused path.  Everything the fused kernels support (L <= 384) goes to
# them first, so this only matters above 384.  Set from the measurement in DESIGN.md section 7 (tools/attention_bench.py).
STREAM_MIN_L = 385


def attention_path(l, dh):
    """'fused' | 'stream' | 'unfused': which implementation attention() uses for sequence length l and head dimension dh"""
    if FLASH_ATTENTION:
        if lib().muvo_attention_supported(l, dh):
            return 'fused'
        if l >= STREAM_MIN_L and lib().muvo_attention_stream_supported(l, dh):
            return 'stream'
    return 'unfused'


_ATTENTION_FNS = {'fused': FlashAttentionFn, 'stream': StreamAttentionFn, 'unfused': AttentionFn}


_MASKED_ATTENTION_FNS = {'fused': MaskedFlashAttentionFn, 'stream': MaskedStreamAttentionFn}


def masked_attention_path(l, dh):
    """'fused' | 'stream': which kernels attention() uses under a key mask.  Resident when it fits, otherwise streamed for any
    l >= 1 (STREAM_MIN_L does not apply: the unfused path has no mask).  ValueError where no fused kernel can run: the mask is
    never dropped silently."""
    if not FLASH_ATTENTION:
        raise ValueError('attention: a key mask needs the fused kernels, which MUVO_FLASH_ATTN=0 turns off')
    if lib().muvo_attention_supported(l, dh):
        return 'fused'
    if lib().muvo_attention_stream_supported(l, dh):
        return 'stream'
    raise ValueError(f'attention: no masked kernel for sequence length {l}, head dimension {dh}')


def key_mask_rows(key_mask, n, l):
    """The (n, l) bool / uint8 device mask as the (n, roundup(l, 16)) contiguous uint8 tensor the kernels read (zero padding);
    a tensor that already is one (what this function returned) comes back as it is"""
    lp = (l + 15) // 16 * 16
    if key_mask.dtype == torch.uint8 and key_mask.is_cuda and tuple(key_mask.shape) == (n, lp) and key_mask.is_contiguous() \
            and key_mask.data_ptr() % 16 == 0:
        return key_mask
    if key_mask.dim() != 2 or tuple(key_mask.shape) != (n, l):
        raise ValueError(f'attention: key_mask must be (N, L) = ({n}, {l}), got {tuple(key_mask.shape)}')
    if key_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f'attention: key_mask must be bool or uint8, got {key_mask.dtype}')
    if not key_mask.is_cuda:
        raise ValueError('attention: key_mask must be on the device')
    rows = torch.zeros(n, lp, dtype=torch.uint8, device=key_mask.device)
    rows[:, :l] = key_mask.to(torch.uint8) if key_mask.dtype == torch.bool else key_mask
    return rows


def attention(qkv, nheads, p, seed, key_mask=None):
    """key_mask: (N, L) bool or uint8 on the device, non-zero = the key is ignored by every query of its frame (torch's
    src_key_padding_mask; not differentiable).  A caller with several attention calls under one mask passes key_mask_rows()'s
    result, which is taken as it is."""
    l, n, e3 = qkv.shape
    if key_mask is None:
        return _ATTENTION_FNS[attention_path(l, e3 // 3 // nheads)].apply(qkv, nheads, p, seed)
    path = masked_attention_path(l, e3 // 3 // nheads)
    return _MASKED_ATTENTION_FNS[path].apply(qkv, nheads, p, seed, key_mask_rows(key_mask, n, l))


# ================================================================================================ RSSM
class GRUPointwiseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gi, gh, h):
        gi, gh, h = gi.contiguous(), gh.contiguous(), h.contiguous()
        b, hd = h.shape
        hn = torch.empty_like(h)
        _ck(lib().muvo_gru_fwd(_f(gi), _f(gh), _f(h), _f(hn), b, hd, _st()))
        ctx.save_for_backward(gi, gh, h)
        return hn

    @staticmethod
    def backward(ctx, dhn):
        gi, gh, h = ctx.saved_tensors
        b, hd = h.shape
        dhn = dhn.contiguous()
        dgi, dgh, dh = torch.empty_like(gi), torch.empty_like(gh), torch.empty_like(h)
        _ck(lib().muvo_gru_bwd(_f(gi), _f(gh), _f(h), _f(dhn), _f(dgi), _f(dgh), _f(dh), b, hd, _st()))
        return dgi, dgh, dh


def gru_pointwise(gi, gh, h):
    return GRUPointwiseFn.apply(gi, gh, h)


class RSSMSampleFn(torch.autograd.Function):
    """(mu|log_sigma) -> mu, sigma = 2*sigmoid(ls/2)+0.1, sample = mu + sigma*eps."""

    @staticmethod
    def forward(ctx, mls, eps, min_std):
        mls = mls.contiguous()
        b, s2 = mls.shape
        s = s2 // 2
        mu, sigma, sample = (torch.empty(b, s, device=mls.device, dtype=torch.float32) for _ in range(3))
        if eps is not None:
            assert eps.stride(-1) == 1 and eps.shape == (b, s)
            eld = eps.stride(0)
            pe = C.c_void_p(eps.data_ptr())
        else:
            eld, pe = 0, None
        _ck(lib().muvo_rssm_sample_fwd(_f(mls), pe, _i64(eld), _f(mu), _f(sigma), _f(sample), b, s, _fl(min_std), _st()))
        ctx.eps = eps
        ctx.save_for_backward(mls)
        return mu, sigma, sample

    @staticmethod
    def backward(ctx, dmu, dsigma, dsample):
        (mls,) = ctx.saved_tensors
        b, s2 = mls.shape
        s = s2 // 2
        eps = ctx.eps
        if eps is not None:
            eld, pe = eps.stride(0), C.c_void_p(eps.data_ptr())
        else:
            eld, pe = 0, None

        def cg(t):
            return None if t is None else t.contiguous()
        dmu, dsigma, dsample = cg(dmu), cg(dsigma), cg(dsample)
        dmls = torch.empty_like(mls)
        _ck(lib().muvo_rssm_sample_bwd(_f(mls), pe, _i64(eld), _f(dmu), _f(dsigma), _f(dsample), _f(dmls), b, s, _st()))
        return dmls, None, None


def rssm_sample(mls, eps, min_std=0.1):
    return RSSMSampleFn.apply(mls, eps, min_std)


def _ptr_table(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        if t is not None:
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
            arr[i] = t.data_ptr()
    return arr


# The pointer tables of muvo_rssm_forward / muvo_rssm_backward by name, in the order of include/muvo_hip.h: the weights with their
# place in the module, the kept and gradient tensors (B, T, .) with the symbol of their last-axis width (_rssm_new).  Plain data:
# tests/test_rssm_reference.py holds it against tests/rssm_reference.py.
RSSM_WEIGHTS = dict(w_pre='pre_gru_net.0.weight', b_pre='pre_gru_net.0.bias', w_ih='recurrent_model.weight_ih',
                    w_hh='recurrent_model.weight_hh', b_ih='recurrent_model.bias_ih', b_hh='recurrent_model.bias_hh',
                    w_pa='prior_action_module.0.weight', b_pa='prior_action_module.0.bias', w_qa='posterior_action_module.0.weight',
                    b_qa='posterior_action_module.0.bias', w_p0='prior.module.0.weight', b_p0='prior.module.0.bias',
                    w_p2='prior.module.2.weight', b_p2='prior.module.2.bias', w_q0='posterior.module.0.weight',
                    b_q0='posterior.module.0.bias', w_q2='posterior.module.2.weight', b_q2='posterior.module.2.bias')
RSSM_KEEP12 = dict(hprev='H', zprev='S', aprev='AD', u='H', gi='3H', gh='3H', xp='HP', xq='HQ', y1p='HP', y1q='HQ', mls_p='2S', mls_q='2S')
RSSM_GRAD10 = dict(d_emb='E', dmls_p='2S', dmls_q='2S', dy1p='HP', dy1q='HQ', dgi='3H', dgh='3H', du='H', dla_p='A', dla_q='A')
# weight gradient = dY^T X over the B T rows, bias gradient = column sums of dY: (dY, X, weight, bias)
RSSM_PARAM_PAIRS = (('du', 'zprev', 'w_pre', 'b_pre'), ('dgi', 'u', 'w_ih', 'b_ih'), ('dgh', 'hprev', 'w_hh', 'b_hh'),
                    ('dla_p', 'aprev', 'w_pa', 'b_pa'), ('dla_q', 'aprev', 'w_qa', 'b_qa'), ('dy1p', 'xp', 'w_p0', 'b_p0'),
                    ('dmls_p', 'y1p', 'w_p2', 'b_p2'), ('dy1q', 'xq', 'w_q0', 'b_q0'), ('dmls_q', 'y1q', 'w_q2', 'b_q2'))


def rssm_weights(rssm):
    """The 18 parameter tensors in the order of RSSM_WEIGHTS."""
    return [rssm.get_parameter(path) for path in RSSM_WEIGHTS.values()]


def _rssm_new(table, dims, dev):
    """{name: empty (B, T, width) tensor} in the order of a table {name: width symbol}"""
    B, T, H, S, E, A, AD = dims
    wd = {'H': H, 'S': S, 'E': E, 'A': A, 'AD': AD, '3H': 3 * H, '2S': 2 * S, 'HP': H + A, 'HQ': H + E + A}
    return {n: torch.empty(B, T, wd[w], device=dev, dtype=torch.float32) for n, w in table.items()}


def _rssm_grid_may_start(dev):
    """deterministic mode runs single-workgroup weight-gradient kernels on the side streams that can hold a compute unit for a long
    time: the persistent grid must not wait for them inside its bounded barrier spin"""
    if get_deterministic():
        join_side_streams(dev)


class RSSMFusedFn(torch.autograd.Function):
    """RSSM.forward (transition.py:76-127) for a whole sequence: one persistent kernel forward, one backward (csrc/rssm.hip),
    then one skinny GEMM per weight for dW = dY^T X over the b*T rows."""

    @staticmethod
    def forward(ctx, emb, act, noise, rssm, mask):
        emb, act, noise = emb.contiguous(), act.contiguous(), noise.contiguous()
        B, T, E = emb.shape
        dims = (B, T, rssm.hidden_state_dim, rssm.state_dim, E, rssm.action_latent_dim, act.shape[-1])
        dev = emb.device
        out = _rssm_new(dict(h='H', mu_p='S', sg_p='S', z_p='S', mu_q='S', sg_q='S', z_q='S'), dims, dev)
        keep = _rssm_new(RSSM_KEEP12, dims, dev)
        bar = rssm_barrier_words(dev)
        rssm_check(dev, post=False)
        _rssm_grid_may_start(dev)
        _ck(lib().muvo_rssm_forward(*dims, _ptr_table(rssm_weights(rssm)), _f(emb), _f(act), _f(noise), C.c_uint64(mask),
                                    _ptr_table(list(out.values())), _ptr_table(list(keep.values())), _p(bar),
                                    _fl(rssm.prior.min_std), _st()))
        if not any(ctx.needs_input_grad):
            rssm_check(dev)        # no backward will follow (validation / imagination): post the error-word copy here
        ctx.rssm, ctx.mask, ctx.dims = rssm, mask, dims
        ctx.save_for_backward(noise, *keep.values())
        return tuple(out.values())

    @staticmethod
    def backward(ctx, *gout):
        noise, *kept = ctx.saved_tensors
        B, T, H, S, E, A, AD = ctx.dims
        dev = noise.device
        L = lib()
        gout = [None if g is None else g.contiguous() for g in gout]
        t = dict(zip(RSSM_KEEP12, kept), **_rssm_new(RSSM_GRAD10, ctx.dims, dev))
        wt = scratch('rssm_wt', L.muvo_rssm_transposed_floats(H, S, E, A), dev)
        sc = scratch('rssm_scratch', L.muvo_rssm_scratch_floats(B, H, S, E, A), dev)
        bar = rssm_barrier_words(dev)
        _rssm_grid_may_start(dev)
        w = dict(zip(RSSM_WEIGHTS, rssm_weights(ctx.rssm)))
        _ck(L.muvo_rssm_backward(*ctx.dims, _ptr_table(list(w.values())), _f(wt), _f(noise), C.c_uint64(ctx.mask),
                                 _ptr_table([t[n] for n in ('hprev', 'gi', 'gh', 'mls_p', 'mls_q')]), _ptr_table(gout),
                                 _ptr_table([t[n] for n in RSSM_GRAD10]), _f(sc), _p(bar), _st()))
        rssm_check(dev)
        rows = B * T
        for dy, x, wn, _ in RSSM_PARAM_PAIRS:
            out_f, in_f = w[wn].shape
            if w[wn].requires_grad:
                gemm(t[dy], t[x], grad_of(w[wn]), out_f, in_f, rows, 1, out_f, in_f, 1, in_f, mode=1)
        for dy, _, _, bn in RSSM_PARAM_PAIRS:
            if w[bn].requires_grad:
                n = w[bn].numel()
                _ck(L.muvo_colsum_acc(_f(t[dy]), _f(grad_of(w[bn])), _i64(rows), _i64(n), _i64(n), _st()))
        return t['d_emb'], None, None, None, None


FUSED_RSSM = os.environ.get('MUVO_FUSED_RSSM', '1') != '0'
_rssm_watch = {}


def rssm_barrier_words(dev):
    """The four 32-bit words the persistent RSSM kernels synchronise through: [0] the grid-barrier counter (reset by every
    launch), [1] the STICKY error word a workgroup raises when its barrier spin times out (the grid was not co-resident)."""
    t = _scratch.get(('rssm_bar', dev, torch.int32))
    if t is None:
        t = _scratch[('rssm_bar', dev, torch.int32)] = torch.zeros(4, device=dev, dtype=torch.int32)
    return t


def rssm_check(dev, post=True):
    """Raise if an earlier fused RSSM launch on `dev` gave up in its grid barrier.  No synchronisation: after a launch
    (`post`) the error word is copied to pinned host memory behind the kernel, an event marks the copy, and a later call looks
    at the host copy once that event has completed - the error surfaces at the latest one step after the failed launch."""
    w = _rssm_watch.get(dev)
    if w is None:
        w = _rssm_watch[dev] = dict(host=torch.zeros(1, dtype=torch.int32).pin_memory(), ev=None)
    if w['ev'] is not None and w['ev'].query():
        if int(w['host'][0]) != 0:
            # the word is sticky on the device (every later fused launch would leave at its first barrier): clear it and the
            # host copy, so that a caller who catches this and switches to MUVO_FUSED_RSSM=0 / a smaller grid can go on
            w['host'].zero_()
            w['ev'] = None
            rssm_barrier_words(dev)[1:2].zero_()
            raise RuntimeError('muvo_rssm: a persistent RSSM kernel timed out in its grid barrier (its workgroups were not '
                               'co-resident: another persistent kernel or a CU mask is holding compute units); set '
                               'MUVO_FUSED_RSSM=0 or lower MUVO_RSSM_GRID')
        w['ev'] = None
    if post and w['ev'] is None:
        w['host'].copy_(rssm_barrier_words(dev)[1:2], non_blocking=True)
        w['ev'] = torch.cuda.Event()
        w['ev'].record(torch.cuda.current_stream(dev))


def rssm_fused_supported(B, T, H, S, E, A, AD):
    return FUSED_RSSM and bool(lib().muvo_rssm_supported(B, T, H, S, E, A, AD))


def rssm_fused(emb, act, noise, rssm, use_prior):
    mask = sum(1 << t for t, f in enumerate(use_prior) if f)
    return RSSMFusedFn.apply(emb, act, noise, rssm, mask)


# ================================================================================================ preprocess (no grad)
def preprocess_image(img_u8, crop, mean, std):
    """(B,S,3,H,W) u8 -> (label (B,S,3,h,w) in [0,1], normalised image)."""
    img_u8 = img_u8.contiguous()
    b, s, c, h, w = img_u8.shape
    left, top, right, bottom = crop
    ch, cw = bottom - top, right - left
    label = torch.empty(b, s, c, ch, cw, device=img_u8.device, dtype=torch.float32)
    norm = torch.empty_like(label)
    m = (C.c_float * 3)(*mean)
    sd = (C.c_float * 3)(*std)
    _ck(lib().muvo_preprocess_image(_p(img_u8), _f(label), _f(norm), _i64(b * s * c), c, h, w, top, left, ch, cw, m, sd,
                                    _st()))
    return label, norm


def resize_bilinear_aa(x, oh, ow, mean=None, std=None):
    """(..., C, H, W) float -> antialiased linear resize to (oh, ow) (torchvision resize(antialias=True)); with mean / std also
    the ImageNet-normalised copy (returns (y, ynorm))."""
    x = x.contiguous()
    c, h, w = x.shape[-3:]
    y = torch.empty(*x.shape[:-2], oh, ow, device=x.device, dtype=torch.float32)
    yn = torch.empty_like(y) if mean is not None else None
    m = (C.c_float * 3)(*mean) if mean is not None else None
    sd = (C.c_float * 3)(*std) if mean is not None else None
    _ck(lib().muvo_resize_bilinear_aa(_f(x), _f(y), _f(yn), m, sd, _i64(x.numel() // (h * w)), c, h, w, oh, ow, _st()))
    return (y, yn) if mean is not None else y


def preprocess_route(route_u8, size, mean, std):
    route_u8 = route_u8.contiguous()
    b, s, c, h, w = route_u8.shape
    out = torch.empty(b, s, c, size, size, device=route_u8.device, dtype=torch.float32)
    m = (C.c_float * 3)(*mean)
    sd = (C.c_float * 3)(*std)
    _ck(lib().muvo_preprocess_route(_p(route_u8), _f(out), _i64(b * s * c), c, h, w, size, size, m, sd, _st()))
    return out


PIXAUG_STRIDE, ROUTEAUG_STRIDE = 16, 8


def pixel_augment(label, norm, params, mean, std):
    """PixelAugmentation (preprocess.py:295-333) on the cropped [0,1] image `label` (b,s,3,h,w), IN PLACE (it is rgb_label_1),
    re-normalising the augmented frames into `norm`.  params: (b*s, PIXAUG_STRIDE) float32 device table (muvo_amd/augment.py)."""
    b, s, c, h, w = label.shape
    assert c == 3 and label.is_contiguous() and norm.is_contiguous() and params.shape == (b * s, PIXAUG_STRIDE)
    tmp = scratch('pixaug_tmp', label.numel(), label.device)
    gsum = scratch('pixaug_gray', b * s, label.device, torch.float64)
    m = (C.c_float * 3)(*mean)
    sd = (C.c_float * 3)(*std)
    _ck(lib().muvo_pixel_augment(_f(label), _f(norm), _f(tmp), _f(params), _p(gsum), _i64(b * s), h, w, m, sd, _st()))


def preprocess_route_aug(route_u8, size, mean, std, params=None):
    """preprocess_route + RouteAugmentation (preprocess.py:336-367); params: (b, ROUTEAUG_STRIDE) float32 device table or None."""
    route_u8 = route_u8.contiguous()
    b, s, c, h, w = route_u8.shape
    out = torch.empty(b, s, c, size, size, device=route_u8.device, dtype=torch.float32)
    m = (C.c_float * 3)(*mean)
    sd = (C.c_float * 3)(*std)
    assert params is None or params.shape == (b, ROUTEAUG_STRIDE)
    _ck(lib().muvo_preprocess_route_aug(_p(route_u8), _f(out), _f(params), b, s, c, h, w, size, size, m, sd, _st()))
    return out


def divide_scalar(x, divisor):
    x = x.contiguous()
    y = torch.empty_like(x)
    _ck(lib().muvo_divide_scalar(_f(x), _f(y), _i64(x.numel()), _fl(divisor), _st()))
    return y


def resize_bilinear(x, oh, ow):
    """x (..., H, W) -> (..., oh, ow), bilinear align_corners=False without antialias."""
    x = x.contiguous()
    h, w = x.shape[-2:]
    y = torch.empty(*x.shape[:-2], oh, ow, device=x.device, dtype=torch.float32)
    _ck(lib().muvo_resize_bilinear(_f(x), _f(y), _i64(x.numel() // (h * w)), h, w, oh, ow, _st()))
    return y


class _ResizeBilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, oh, ow):
        ctx.in_hw = tuple(x.shape[-2:])
        return resize_bilinear(x, oh, ow)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        h, w = ctx.in_hw
        oh, ow = g.shape[-2:]
        dx = torch.empty(*g.shape[:-2], h, w, device=g.device, dtype=torch.float32)
        _ck(lib().muvo_resize_bilinear_bwd(_f(g), _f(dx), _i64(g.numel() // (oh * ow)), h, w, oh, ow, _st()))
        return dx, None, None


def interpolate_bilinear(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=False) with autograd (common.py:96)."""
    return _ResizeBilinearFn.apply(x, int(size[0]), int(size[1]))


class _SoftmaxChannelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        B, C = x.shape[:2]
        y = torch.empty_like(x)
        _ck(lib().muvo_softmax_channel_fwd(_f(x), _f(y), B, C, _i64(x[0, 0].numel()), _st()))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        B, C = y.shape[:2]
        dx = torch.empty_like(y)
        _ck(lib().muvo_softmax_channel_bwd(_f(y), _f(g.contiguous()), _f(dx), B, C, _i64(y[0, 0].numel()), _st()))
        return dx


def instance_labels(instance_label, sigma, ignore_index=255):
    """convert_instance_mask_to_center_and_offset_label (instance_utils.py:4-35): instance ids (b, s, 1, h, w) ->
    center (b, s, 1, h, w), offset (b, s, 2, h, w) float32."""
    b, s, _, h, w = instance_label.shape
    inst = instance_label.to(torch.uint8).contiguous()
    center = torch.empty(b, s, 1, h, w, device=inst.device, dtype=torch.float32)
    offset = torch.empty(b, s, 2, h, w, device=inst.device, dtype=torch.float32)
    scratch = torch.empty(b * s * 256 * 3, device=inst.device, dtype=torch.float64)
    _ck(lib().muvo_instance_labels(_p(inst), _i64(b * s), h, w, _fl(sigma), _fl(ignore_index), _p(scratch), _f(center), _f(offset), _st()))
    return center, offset


def softmax_channel(x):
    """x.softmax(dim=1) of an (B, C, ...) tensor (mile.py:509)."""
    return _SoftmaxChannelFn.apply(x)


def resize_nearest(x, out_sz):
    """nearest resize of the trailing len(out_sz) dims (2 or 3), float32 or uint8."""
    x = x.contiguous()
    nd = len(out_sz)
    in_sz = tuple(x.shape[-nd:])
    i3 = (1,) * (3 - nd) + in_sz
    o3 = (1,) * (3 - nd) + tuple(out_sz)
    y = torch.empty(*x.shape[:-nd], *out_sz, device=x.device, dtype=x.dtype)
    nc = x.numel() // (i3[0] * i3[1] * i3[2])
    fn = lib().muvo_resize_nearest_u8 if x.dtype == torch.uint8 else lib().muvo_resize_nearest_f32
    assert x.dtype in (torch.uint8, torch.float32)
    _ck(fn(_p(x), _p(y), _i64(nc), *i3, *o3, _st()))
    return y


# ================================================================================================ losses
def _grad_vector(gs, device):
    """the gradients of k scalar outputs of a loss Function (`terms=True`: returned as separate 0-d tensors, so that the caller's
    `[i]` is a tuple index and not k select_backward nodes of 2-3 launches each) as ONE (k,) device vector for the backward kernel;
    a term nobody differentiated counts as zero.  One launch (all terms usually receive the same upstream scalar).  The gradient
    of the stacked 1-D output (`terms=False`) is that vector already."""
    if len(gs) == 1 and gs[0] is not None and gs[0].dim() == 1:
        return gs[0].contiguous()
    first = next((g for g in gs if g is not None), None)
    if first is None:
        return torch.zeros(len(gs), device=device, dtype=torch.float32)
    if all(g is first for g in gs):
        return first.reshape(1).expand(len(gs)).contiguous()
    zero = None
    parts = []
    for g in gs:
        if g is None:
            zero = torch.zeros((), device=device, dtype=torch.float32) if zero is None else zero
            g = zero
        parts.append(g.reshape(()))
    return torch.stack(parts)


def _grad_scalar(g, device):
    """the gradient of the one scalar output of a loss Function as a (1,) device vector; nobody differentiated it: zero"""
    return torch.zeros(1, device=device) if g is None else g.reshape(1)


def _voxel_dims(logits, labels=None):
    """(F, C, V) of logits (B,S,C,X,Y,Z); with labels, also checks that they are the uint8 grid of the logits"""
    b, s, c = logits.shape[:3]
    f = b * s
    v = logits.numel() // (f * c)
    assert labels is None or (labels.dtype == torch.uint8 and labels.numel() == f * v), 'labels must be uint8 (B,S,1,X,Y,Z) on the grid of the logits'
    return f, c, v


def _as_terms(ctx, t, terms):
    if not terms:
        return t
    ctx.set_materialize_grads(False)
    return tuple(t[i] for i in range(t.numel()))


class SpatialLossFn(torch.autograd.Function):
    """weight * SpatialRegressionLoss(norm) over channel ranges of (B,S,C,H,W) tensors.

    `parts` = list of (c0, c1, norm, weight); returns one scalar per part (stacked 1-D tensor)."""

    @staticmethod
    def forward(ctx, pred, target, parts, ignore, mask=None, terms=False):
        # mask: optional explicit (B, S, 1, H, W) uint8 / bool pixel mask (SpatialRegressionLoss(..., instance_mask), losses.py:87-90)
        pred, target = pred.contiguous(), target.contiguous()
        b, s, c, h, w = pred.shape
        f, hw = b * s, h * w
        if mask is not None:
            mask = mask.to(torch.uint8).contiguous()
            assert mask.numel() == f * hw
        losses = torch.empty(len(parts), device=pred.device, dtype=torch.float32)
        stats = torch.empty(len(parts), 2, device=pred.device, dtype=torch.float64)
        for i, (c0, c1, norm, weight) in enumerate(parts):
            _ck(lib().muvo_spatial_loss_masked_fwd(_f(pred), _f(target), _p(mask), _i64(f), c, _i64(hw), c0, c1, norm, _fl(ignore),
                                                   _fl(weight), C.c_void_p(stats.data_ptr() + 16 * i),
                                                   C.c_void_p(losses.data_ptr() + 4 * i), _st()))
        ctx.parts, ctx.ignore, ctx.dims = parts, ignore, (f, c, hw)
        ctx.save_for_backward(pred, target, stats, mask)
        return _as_terms(ctx, losses, terms)

    @staticmethod
    def backward(ctx, *gs):
        pred, target, stats, mask = ctx.saved_tensors
        f, c, hw = ctx.dims
        g = _grad_vector(gs, pred.device)
        covered = sum(c1 - c0 for c0, c1, _, _ in ctx.parts)
        dpred = torch.empty_like(pred) if covered == c else torch.zeros_like(pred)
        for i, (c0, c1, norm, weight) in enumerate(ctx.parts):
            _ck(lib().muvo_spatial_loss_masked_bwd(_f(pred), _f(target), _p(mask), _f(dpred), _i64(f), c, _i64(hw), c0, c1, norm,
                                                   _fl(ctx.ignore), _fl(weight), C.c_void_p(stats.data_ptr() + 16 * i),
                                                   C.c_void_p(g.data_ptr() + 4 * i), _st()))
        return dpred, None, None, None, None, None


def spatial_losses(pred, target, parts, ignore=255.0, mask=None, terms=False):
    """terms=True: a tuple of 0-d tensors (one per part) instead of the stacked 1-D tensor"""
    return SpatialLossFn.apply(pred, target, parts, ignore, mask, terms)


class VoxelLossFn(torch.autograd.Function):
    """(weight*CE mean, weight*SemScal, weight*GeoScal) for logits (B,S,C,X,Y,Z), labels u8 (B,S,1,X,Y,Z)."""

    @staticmethod
    def forward(ctx, logits, target, weight, class_w, terms=False):
        logits, target = logits.contiguous(), target.contiguous()
        f, c, v = _voxel_dims(logits)
        L = lib()
        stats = torch.empty(L.muvo_voxel_loss_stats_doubles(c), device=logits.device, dtype=torch.float64)
        coef = torch.empty(L.muvo_voxel_loss_coef_floats(c), device=logits.device, dtype=torch.float32)
        loss3 = torch.empty(3, device=logits.device, dtype=torch.float32)
        _ck(L.muvo_voxel_loss_fwd(_f(logits), _p(target), _i64(f), c, _i64(v), _f(class_w), _fl(weight), _p(stats),
                                  _f(coef), _f(loss3), _st()))
        ctx.dims, ctx.weight, ctx.class_w = (f, c, v), weight, class_w
        ctx.save_for_backward(logits, target, coef)
        return _as_terms(ctx, loss3, terms)

    @staticmethod
    def backward(ctx, *gs):
        logits, target, coef = ctx.saved_tensors
        f, c, v = ctx.dims
        g = _grad_vector(gs, logits.device)
        dl = torch.empty_like(logits)
        _ck(lib().muvo_voxel_loss_bwd(_f(logits), _p(target), _f(dl), _i64(f), c, _i64(v), _f(ctx.class_w),
                                      _fl(ctx.weight), _f(coef), _f(g), _st()))
        return dl, None, None, None, None


def voxel_losses(logits, target, weight, class_w=None, terms=False):
    return VoxelLossFn.apply(logits, target, weight, class_w, terms)


class L1RowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight, terms=False):
        pred, target = pred.contiguous(), target.contiguous()
        cols = pred.shape[-1]
        rows = pred.numel() // cols
        loss = torch.empty(1, device=pred.device, dtype=torch.float32)
        _ck(lib().muvo_l1_rows_fwd(_f(pred), _f(target), _i64(rows), cols, _fl(weight), _f(loss), _st()))
        ctx.dims, ctx.weight = (rows, cols), weight
        ctx.save_for_backward(pred, target)
        return _as_terms(ctx, loss, terms)

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        rows, cols = ctx.dims
        dp = torch.empty_like(pred)
        g = _grad_scalar(g, pred.device)
        _ck(lib().muvo_l1_rows_bwd(_f(pred), _f(target), _f(dp), _i64(rows), cols, _fl(ctx.weight), _f(g.contiguous()),
                                   _st()))
        return dp, None, None, None


class _SegCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, class_w):
        logits = logits.contiguous()
        N, Cc = logits.shape[:2]
        HW = logits[0, 0].numel()
        loss = torch.empty(N, HW, device=logits.device, dtype=torch.float32)
        _ck(lib().muvo_seg_ce_fwd(_f(logits), _p(target), _f(class_w), _f(loss), _i64(N), Cc, _i64(HW), _st()))
        ctx.save_for_backward(logits, target, class_w)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, target, class_w = ctx.saved_tensors
        N, Cc = logits.shape[:2]
        HW = logits[0, 0].numel()
        d = torch.empty_like(logits)
        _ck(lib().muvo_seg_ce_bwd(_f(logits), _p(target), _f(class_w), _f(g.contiguous()), _f(d), _i64(N), Cc, _i64(HW), _st()))
        return d, None, None


def seg_ce_pixel_loss(logits, target, class_w=None):
    """F.cross_entropy(logits (N, C, ...), target (N, ...), weight=class_w, reduction='none') flattened to (N, HW)."""
    t = target.reshape(target.shape[0], -1).to(torch.uint8).contiguous()
    return _SegCEFn.apply(logits.float(), t, class_w)


def l1_rows_loss(pred, target, weight, terms=False):
    return L1RowsFn.apply(pred, target, weight, terms)


class KLLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pm, ps, qm, qs, weight, alpha, terms=False):
        pm, ps, qm, qs = (t.contiguous() for t in (pm, ps, qm, qs))
        b, t, s = pm.shape
        loss = torch.empty(1, device=pm.device, dtype=torch.float32)
        _ck(lib().muvo_kl_loss_fwd(_f(pm), _f(ps), _f(qm), _f(qs), b, t, s, _fl(weight), _f(loss), _st()))
        ctx.args = (b, t, s, weight, alpha)
        ctx.save_for_backward(pm, ps, qm, qs)
        return _as_terms(ctx, loss, terms)

    @staticmethod
    def backward(ctx, g):
        pm, ps, qm, qs = ctx.saved_tensors
        b, t, s, weight, alpha = ctx.args
        g = _grad_scalar(g, pm.device)
        d = [torch.empty_like(pm) for _ in range(4)]
        _ck(lib().muvo_kl_loss_bwd(_f(pm), _f(ps), _f(qm), _f(qs), _f(d[0]), _f(d[1]), _f(d[2]), _f(d[3]), b, t, s,
                                   _fl(weight), _fl(alpha), _f(g.contiguous()), _st()))
        return d[0], d[1], d[2], d[3], None, None, None


def kl_loss(pm, ps, qm, qs, weight, alpha, terms=False):
    return KLLossFn.apply(pm, ps, qm, qs, weight, alpha, terms)


def _chamfer_forward(pred, target, weight, with_indices):
    pred, target = pred.contiguous(), target.contiguous()
    b, s, cp, h, w = pred.shape
    ct = target.shape[2]
    assert target.shape[:2] == (b, s) and target.shape[3:] == (h, w), 'prediction and target must hold the same number of points'
    f, n = b * s, h * w
    L = lib()
    ws = torch.empty(max(1, L.muvo_chamfer_loss_ws_doubles(_i64(f), _i64(n))), device=pred.device, dtype=torch.float64)
    idx = torch.empty(2, f, n, device=pred.device, dtype=torch.int32) if with_indices else None
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    _ck(L.muvo_chamfer_loss_fwd(_f(pred), _f(target), _i64(f), cp, ct, _i64(n), _fl(weight), _p(ws),
                                _p(idx[0]) if with_indices else _p(None), _p(idx[1]) if with_indices else _p(None), _f(loss), _st()))
    return pred, target, loss, idx, (f, cp, ct, n)


class ChamferLossFn(torch.autograd.Function):
    """weight * CDLoss (muvo/losses.py:352-367, reducer = mean) between the points of two (B,S,C,H,W) tensors: x, y, z are
    channels 0..2, further channels are never read (C may differ between the two).  The gradient goes to the prediction only;
    its channels >= 3 are exactly zero.  The nearest-neighbour indices are kept only when a backward can follow: under
    torch.no_grad() the search writes none, and the value is bit-identical."""

    @staticmethod
    def forward(ctx, pred, target, weight, terms=False, grad_enabled=True):
        # grad_enabled: the caller's grad mode (inside forward it is always off, and needs_input_grad stays True under no_grad)
        need = ctx.needs_input_grad[0] and grad_enabled
        pred, target, loss, idx, (f, cp, ct, n) = _chamfer_forward(pred, target, weight, need)
        ctx.dims, ctx.weight = (f, cp, ct, n), weight
        if need:
            ctx.save_for_backward(pred, target, idx)
        return _as_terms(ctx, loss, terms)

    @staticmethod
    def backward(ctx, g):
        pred, target, idx = ctx.saved_tensors
        f, cp, ct, n = ctx.dims
        g = _grad_scalar(g, pred.device)
        dpred = torch.empty_like(pred)
        _ck(lib().muvo_chamfer_loss_bwd(_f(pred), _f(target), _p(idx[0]), _p(idx[1]), _f(dpred), _i64(f), cp, ct, _i64(n),
                                        _fl(ctx.weight), _f(g.contiguous()), _st()))
        return dpred, None, None, None, None


def chamfer_loss(pred, target, weight, terms=False):
    """terms=True: a 1-tuple holding the 0-d loss instead of the (1,) tensor (as the other loss entry points)"""
    return ChamferLossFn.apply(pred, target, weight, terms, torch.is_grad_enabled())


def chamfer_nearest(pred, target):
    """The selections the loss differentiates, (2, B*S, n) int32: [0][f, i] = the target point nearest to prediction point i,
    [1][f, j] = the prediction point nearest to target point j (lowest index on a tie)."""
    return _chamfer_forward(pred.detach(), target.detach(), 1.0, True)[3]


def _lovasz_forward(logits, labels, weight, with_dlde, with_errors=False):
    logits, labels = logits.contiguous(), labels.contiguous()
    f, c, v = _voxel_dims(logits, labels)
    L = lib()
    ws = torch.empty(max(16, L.muvo_lovasz_ws_bytes(_i64(f), c, _i64(v))), device=logits.device, dtype=torch.uint8)
    errors = torch.empty(f, c, v, device=logits.device, dtype=torch.float32) if with_errors else None
    dlde = torch.empty(f, c, v, device=logits.device, dtype=torch.float32) if with_dlde else None
    present = torch.empty(f, c, device=logits.device, dtype=torch.uint8)
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    _ck(L.muvo_lovasz_fwd(_f(logits), _p(labels), _i64(f), c, _i64(v), _fl(weight), _p(ws), _f(errors), _f(dlde), _p(present),
                          _f(loss), _st()))
    return logits, labels, loss, errors, dlde, present, ws, (f, c, v)


class VoxelLovaszFn(torch.autograd.Function):
    """weight * Lovasz-softmax loss for logits (B,S,C,X,Y,Z), labels u8 (B,S,1,X,Y,Z); labels >= C are
    ignored.  Every frame is a segment of its own, classes 'present'.  The per-rank Jaccard increments are kept, in voxel order,
    only when a backward can follow: under torch.no_grad() none are written, and the value is bit-identical."""

    @staticmethod
    def forward(ctx, logits, labels, weight, terms=False, grad_enabled=True):
        need = ctx.needs_input_grad[0] and grad_enabled
        logits, labels, loss, _, dlde, present, _, dims = _lovasz_forward(logits, labels, weight, need)
        ctx.dims, ctx.weight = dims, weight
        if need:
            ctx.save_for_backward(logits, labels, dlde, present)
        return _as_terms(ctx, loss, terms)

    @staticmethod
    def backward(ctx, g):
        logits, labels, dlde, present = ctx.saved_tensors
        f, c, v = ctx.dims
        g = _grad_scalar(g, logits.device)
        dl = torch.empty_like(logits)
        _ck(lib().muvo_lovasz_bwd(_f(logits), _p(labels), _f(dlde), _p(present), _f(dl), _i64(f), c, _i64(v), _fl(ctx.weight),
                                  _f(g.contiguous()), _st()))
        return dl, None, None, None, None


def voxel_lovasz_loss(logits, labels, weight, terms=False):
    """terms=True: a 1-tuple holding the 0-d loss instead of the (1,) tensor (as the other loss entry points)"""
    return VoxelLovaszFn.apply(logits, labels, weight, terms, torch.is_grad_enabled())


def voxel_lovasz_parts(logits, labels):
    """What the loss is made of, for tests and the benchmark: (errors (F,C,V), dlde (F,C,V), present (F,C) uint8,
    frame_class_loss (F,C) float64 = L_fc, unweighted) for logits (B,S,C,...) and labels u8 (B,S,1,...)."""
    _, _, _, errors, dlde, present, ws, (f, c, v) = _lovasz_forward(logits.detach(), labels, 1.0, True, True)
    return errors, dlde, present, ws[:f * c * 8].view(torch.float64).view(f, c).clone()


def _render_ws(f, v, r, device):
    n = int(lib().muvo_render_ws_bytes(_i64(f), _i64(v), _i64(r)))
    if n < 0:
        raise ValueError(f'voxel_render_loss: {f} frames of {v} voxels and {r} rays (1..65535 frames, fewer than 2^30 voxels, 1..2^24 rays)')
    return torch.empty(max(16, n), device=device, dtype=torch.uint8), n


def _render_label_pass(logits, labels, rays):
    """What both rendered losses start with: the contiguous inputs, their sizes, and muvo_raycast's (hit, t) of the table's rays
    through the label grid."""
    logits, labels = logits.contiguous(), labels.contiguous()
    assert logits.dim() == 6 and logits.dtype == torch.float32, 'logits must be float32 (B,S,C,X,Y,Z)'
    f, c, v = _voxel_dims(logits, labels)
    X, Y, Z = (int(n) for n in logits.shape[3:])
    assert rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 7 and rays.is_contiguous() and rays.device == logits.device, \
        'rays must be a contiguous float32 (R, 7) table on the device of the logits'
    R = int(rays.shape[0])
    grid, bricks = raycast_bricks(labels.view(f, X, Y, Z))          # occupied = class != 0, as for the metric
    hit, lt, _ = raycast(grid, bricks, rays)
    return logits, grid, hit, lt, (f, c, X, Y, Z, R)


def _render_forward(logits, labels, rays, n_valid, weight, parts=False):
    logits, _, hit, lt, (f, c, X, Y, Z, R) = _render_label_pass(logits, labels, rays)
    v = X * Y * Z
    dev = logits.device
    ws, ws_bytes = _render_ws(f, v, R, dev)
    depth = torch.empty(f, R, device=dev, dtype=torch.float64)
    target = torch.empty(f, R, device=dev, dtype=torch.float32)
    t_last = torch.empty(f, R, device=dev, dtype=torch.float32) if parts else None
    cells = torch.empty(f, R, device=dev, dtype=torch.int32) if parts else None
    t_exit = torch.empty(f, R, device=dev, dtype=torch.float32) if parts else None
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    _ck(lib().muvo_render_fwd(_f(logits), _i64(f), c, X, Y, Z, _f(rays), _i64(R), _i64(n_valid), _p(hit), _f(lt), _fl(weight), _p(ws), _i64(ws_bytes),
                              _p(depth), _f(target), _f(t_last), _p(cells), _f(t_exit), _f(loss), _st()))
    return logits, loss, depth, target, t_last, cells, t_exit, (f, c, X, Y, Z, R)


class VoxelRenderFn(torch.autograd.Function):
    """weight * rendered first-hit depth loss (include/muvo_hip.h: muvo_render_fwd) for logits
    (B,S,C,X,Y,Z), labels u8 (B,S,1,X,Y,Z) and a ray table (R, 7) in grid units with `n_valid` valid rays.  Kept for the backward
    pass: the logits (q and a are recomputed), D (F, R) float64 and the label's t* (F, R)."""

    @staticmethod
    def forward(ctx, logits, labels, rays, n_valid, weight, terms=False, grad_enabled=True):
        need = ctx.needs_input_grad[0] and grad_enabled
        logits, loss, depth, target, _, _, _, dims = _render_forward(logits, labels, rays, n_valid, weight)
        ctx.dims, ctx.weight, ctx.n_valid = dims, weight, int(n_valid)
        if need:
            ctx.save_for_backward(logits, rays, depth, target)
        return _as_terms(ctx, loss, terms)

    @staticmethod
    def backward(ctx, g):
        logits, rays, depth, target = ctx.saved_tensors
        f, c, X, Y, Z, R = ctx.dims
        g = _grad_scalar(g, logits.device)
        ws, ws_bytes = _render_ws(f, X * Y * Z, R, logits.device)
        dl = torch.empty_like(logits)
        _ck(lib().muvo_render_bwd(_f(logits), _i64(f), c, X, Y, Z, _f(rays), _i64(R), _i64(ctx.n_valid), _p(depth), _f(target), _fl(ctx.weight),
                                  _f(g.contiguous()), _p(ws), _i64(ws_bytes), _f(dl), _st()))
        return dl, None, None, None, None, None, None


def voxel_render_loss(logits, labels, rays, n_valid, weight, terms=False):
    """terms=True: a 1-tuple holding the 0-d loss instead of the (1,) tensor (as the other loss entry points)"""
    return VoxelRenderFn.apply(logits, labels, rays, n_valid, weight, terms, torch.is_grad_enabled())


def voxel_render_parts(logits, labels, rays, n_valid, weight=1.0):
    """What the loss is made of, for tests and the benchmark: (loss (1,), D (F, R) float64, t* (F, R), T_n (F, R), cells per ray
    (F, R) int32 with -1 at invalid rays, t_exit (F, R)).  The march runs to the end of every ray here; the loss has the bits
    of voxel_render_loss."""
    _, loss, depth, target, t_last, cells, t_exit, _ = _render_forward(logits.detach(), labels, rays, n_valid, weight, True)
    return loss, depth, target, t_last, cells, t_exit


def _render_class_ws(f, c, v, r, device):
    n = int(lib().muvo_render_class_ws_bytes(_i64(f), c, _i64(v), _i64(r)))
    if n < 0:
        raise ValueError(f'voxel_render_class_loss: {f} frames of {c} classes, {v} voxels and {r} rays (1..65535 frames, 2..16 classes, '
                         'fewer than 2^30 voxels, 1..2^24 rays)')
    return torch.empty(max(16, n), device=device, dtype=torch.uint8), n        # from the caching allocator, as _render_ws


def _render_class_forward(logits, labels, rays, n_valid, weight, parts=False):
    logits, grid, hit, _, (f, c, X, Y, Z, R) = _render_label_pass(logits, labels, rays)
    dev = logits.device
    ws, ws_bytes = _render_class_ws(f, c, X * Y * Z, R, dev)
    mass = torch.empty(f, R, device=dev, dtype=torch.float64)
    target = torch.empty(f, R, device=dev, dtype=torch.int32)
    t_last = torch.empty(f, R, device=dev, dtype=torch.float32) if parts else None
    cells = torch.empty(f, R, device=dev, dtype=torch.int32) if parts else None
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    _ck(lib().muvo_render_class_fwd(_f(logits), _p(grid), _i64(f), c, X, Y, Z, _f(rays), _i64(R), _i64(n_valid), _p(hit), _fl(weight), _p(ws),
                                    _i64(ws_bytes), _p(mass), _p(target), _f(t_last), _p(cells), _f(loss), _st()))
    return logits, loss, mass, target, t_last, cells, (f, c, X, Y, Z, R)


class VoxelRenderClassFn(torch.autograd.Function):
    """weight * rendered first-hit class loss (include/muvo_hip.h: muvo_render_class_fwd) for logits
    (B,S,C,X,Y,Z), labels u8 (B,S,1,X,Y,Z) and a ray table (R, 7) in grid units with `n_valid` valid rays.  A label class >= C at a
    ray's first hit makes the loss ignore that ray (the labels stay on the device: nothing is read back to refuse them).  Kept
    for the backward pass: the logits (the probabilities are recomputed), S_y (F, R) float64 and y (F, R) int32."""

    @staticmethod
    def forward(ctx, logits, labels, rays, n_valid, weight, terms=False, grad_enabled=True):
        need = ctx.needs_input_grad[0] and grad_enabled
        logits, loss, mass, target, _, _, dims = _render_class_forward(logits, labels, rays, n_valid, weight)
        ctx.dims, ctx.weight, ctx.n_valid = dims, weight, int(n_valid)
        if need:
            ctx.save_for_backward(logits, rays, mass, target)
        return _as_terms(ctx, loss, terms)

    @staticmethod
    def backward(ctx, g):
        logits, rays, mass, target = ctx.saved_tensors
        f, c, X, Y, Z, R = ctx.dims
        g = _grad_scalar(g, logits.device)
        ws, ws_bytes = _render_class_ws(f, c, X * Y * Z, R, logits.device)
        dl = torch.empty_like(logits)
        _ck(lib().muvo_render_class_bwd(_f(logits), _i64(f), c, X, Y, Z, _f(rays), _i64(R), _i64(ctx.n_valid), _p(mass), _p(target), _fl(ctx.weight),
                                        _f(g.contiguous()), _p(ws), _i64(ws_bytes), _f(dl), _st()))
        return dl, None, None, None, None, None, None


def voxel_render_class_loss(logits, labels, rays, n_valid, weight, terms=False):
    """terms=True: a 1-tuple holding the 0-d loss instead of the (1,) tensor (as the other loss entry points)"""
    return VoxelRenderClassFn.apply(logits, labels, rays, n_valid, weight, terms, torch.is_grad_enabled())


def voxel_render_class_parts(logits, labels, rays, n_valid, weight=1.0):
    """What the loss is made of, for tests and the benchmark: (loss (1,), S_y (F, R) float64, y (F, R) int32 with -1 at invalid and
    ignored rays, T_n (F, R), cells per ray (F, R) int32 with -1 at invalid rays).  The march runs to the end of every ray here;
    the loss has the bits of voxel_render_class_loss."""
    _, loss, mass, target, t_last, cells, _ = _render_class_forward(logits.detach(), labels, rays, n_valid, weight, True)
    return loss, mass, target, t_last, cells


# ---- distance transform of voxel grids, boundary loss, voxel Chamfer counts (csrc/edt.hip; include/muvo_hip.h: muvo_voxel_edt) ----
def voxel_edt(grid, cap):
    """edt2 (F, X, Y, Z) int32 of a class grid (F, X, Y, Z) uint8: per cell min(cap, the squared distance in cells to the nearest
    occupied cell (1..254) of its frame); `cap` everywhere in a frame without one.  cap >= X^2 + Y^2 + Z^2: untruncated."""
    if grid.dtype != torch.uint8 or grid.dim() != 4:
        raise ValueError(f'voxel_edt: a class grid (F, X, Y, Z) uint8, got {tuple(grid.shape)} {grid.dtype}')
    grid = grid.contiguous()
    F, X, Y, Z = (int(v) for v in grid.shape)
    cap = int(cap)
    n = int(lib().muvo_voxel_edt_ws_bytes(_i64(F), X, Y, Z)) if min(X, Y, Z) >= 1 and max(X, Y, Z) < 2 ** 31 else -1
    if n < 0 or not 1 <= cap < 2 ** 31:
        raise ValueError(f'voxel_edt: {F} frames of {X} x {Y} x {Z} with cap {cap} (1..65535 frames, every axis >= 1, '
                         'X^2 + Y^2 + Z^2 < 2^31, fewer than 2^36 cells, 1 <= cap < 2^31)')
    ws = torch.empty(max(4, n), device=grid.device, dtype=torch.uint8)
    out = torch.empty((F, X, Y, Z), device=grid.device, dtype=torch.int32)
    _ck(lib().muvo_voxel_edt(_p(grid), _i64(F), X, Y, Z, C.c_int32(cap), _p(ws), _i64(n), _p(out), _st()))
    return out


def _boundary_forward(logits, labels, truncate_cells, weight):
    logits, labels = logits.contiguous(), labels.contiguous()
    assert logits.dim() == 6 and logits.dtype == torch.float32, 'logits must be float32 (B,S,C,X,Y,Z)'
    f, c, v = _voxel_dims(logits, labels)
    X, Y, Z = (int(n) for n in logits.shape[3:])
    T = int(truncate_cells)
    n = int(lib().muvo_voxel_boundary_ws_bytes(_i64(f), _i64(v)))
    if n < 0 or not 2 <= c <= 16 or not 1 <= T <= 46340 or max(X, Y, Z) > 2048:
        raise ValueError(f'voxel_boundary_loss: {f} frames of {c} classes on {X} x {Y} x {Z} with a truncation of {T} cells (1..65535 frames, '
                         '2..16 classes, 1..2048 per axis, fewer than 2^30 voxels, 1..46340 cells)')
    dev = logits.device
    pred = raycast_bricks(logits.detach().view(f, c, X, Y, Z))[0]
    edt_label = voxel_edt(labels.view(f, X, Y, Z), T * T)
    edt_pred = voxel_edt(pred, T * T)
    ws = torch.empty(max(16, n), device=dev, dtype=torch.uint8)
    n_g = torch.empty(f + 1, device=dev, dtype=torch.int32)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    _ck(lib().muvo_voxel_boundary_forward(_f(logits), _p(labels), _p(edt_label), _p(edt_pred), _i64(f), c, X, Y, Z, T, _fl(weight), _p(ws), _i64(n),
                                          _p(n_g), _f(loss), _st()))
    return logits, labels, loss, edt_label, edt_pred, pred, n_g, (f, c, X, Y, Z, T)


class VoxelBoundaryFn(torch.autograd.Function):
    """weight * distance-transform boundary loss (include/muvo_hip.h: muvo_voxel_boundary_forward) for logits
    (B,S,C,X,Y,Z), labels u8 (B,S,1,X,Y,Z) and a truncation in cells.  The prediction's class grid and its transform are constants
    of the backward pass.  Kept for it: the logits (the probabilities are recomputed), the labels, both transforms and n_G."""

    @staticmethod
    def forward(ctx, logits, labels, truncate_cells, weight, terms=False, grad_enabled=True):
        need = ctx.needs_input_grad[0] and grad_enabled
        logits, labels, loss, edt_label, edt_pred, _, n_g, dims = _boundary_forward(logits, labels, truncate_cells, weight)
        ctx.dims, ctx.weight = dims, weight
        if need:
            ctx.save_for_backward(logits, labels, edt_label, edt_pred, n_g)
        return _as_terms(ctx, loss, terms)

    @staticmethod
    def backward(ctx, g):
        logits, labels, edt_label, edt_pred, n_g = ctx.saved_tensors
        f, c, X, Y, Z, T = ctx.dims
        g = _grad_scalar(g, logits.device)
        dl = torch.empty_like(logits)
        _ck(lib().muvo_voxel_boundary_backward(_f(logits), _p(labels), _p(edt_label), _p(edt_pred), _p(n_g), _i64(f), c, X, Y, Z, T, _fl(ctx.weight),
                                               _f(g.contiguous()), _f(dl), _st()))
        return dl, None, None, None, None, None


def voxel_boundary_loss(logits, labels, truncate_cells, weight, terms=False):
    """terms=True: a 1-tuple holding the 0-d loss instead of the (1,) tensor (as the other loss entry points)"""
    return VoxelBoundaryFn.apply(logits, labels, truncate_cells, weight, terms, torch.is_grad_enabled())


def voxel_boundary_parts(logits, labels, truncate_cells):
    """What the loss is made of, for tests and the benchmark: (edt2 of the label (F, X, Y, Z) int32, edt2 of the prediction, the
    prediction's class grid (F, X, Y, Z) uint8, n_G (F,) int32), both transforms capped at truncate_cells^2."""
    _, _, _, edt_label, edt_pred, pred, n_g, _ = _boundary_forward(logits.detach(), labels, truncate_cells, 1.0)
    return edt_label, edt_pred, pred, n_g[:-1].clone()


def voxel_cd_counts(label, pred_grid, thresholds2, counts, sums):
    """counts (10,) int64 - frames, skipped frames, n_P, n_G, hits_P[3], hits_G[3] - and sums (2,) float64 - sum_PG, sum_GP - on the
    device are added to, over the F frames of the class grids label and pred_grid (F, X, Y, Z) uint8, from their untruncated
    distance transforms (include/muvo_hip.h: muvo_voxel_cd_counts); thresholds2: three squared distances in cells, integers.
    Nothing is read back."""
    for t in (label, pred_grid):
        assert t.dtype == torch.uint8 and t.dim() == 4, 'voxel_cd_counts: class grids (F, X, Y, Z) uint8'
    label, pred_grid = label.contiguous(), pred_grid.contiguous()
    assert label.shape == pred_grid.shape and label.device == pred_grid.device, 'voxel_cd_counts: label and prediction of one shape'
    F, X, Y, Z = (int(v) for v in label.shape)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (10,) and counts.is_contiguous() and counts.device == label.device
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (2,) and sums.is_contiguous() and sums.device == label.device
    thr = [int(v) for v in thresholds2]
    assert len(thr) == 3, 'voxel_cd_counts: three squared thresholds'
    n = int(lib().muvo_voxel_cd_ws_bytes(_i64(F), _i64(X * Y * Z)))
    if n < 0 or max(X, Y, Z) > 2048:
        raise ValueError(f'voxel_cd_counts: {F} frames of {X} x {Y} x {Z} (1..65535 frames, 1..2048 per axis, fewer than 2^30 voxels)')
    cap = X * X + Y * Y + Z * Z
    edt_label, edt_pred = voxel_edt(label, cap), voxel_edt(pred_grid, cap)
    ws = torch.empty(max(1, n // 8), device=label.device, dtype=torch.float64)
    _ck(lib().muvo_voxel_cd_counts(_p(label), _p(pred_grid), _p(edt_label), _p(edt_pred), _i64(F), X, Y, Z, (C.c_int32 * 3)(*thr), _p(counts), _p(sums),
                                   _p(ws), _i64(n), _st()))


# ================================================================================================ BEV instances, panoptic quality
def bev_instance_decode(center, offset, logits=None, foreground=None, threshold=0.1, radius=1, max_centres=100, thing_classes=(3, 4)):
    """Instances from the centre / offset heads (include/muvo_hip.h: muvo_bev_instance_decode): center (F, H, W) fp32, offset
    (F, 2, H, W) fp32 and either logits (F, C, H, W) fp32 with the thing classes or a foreground mask (F, H, W) uint8 ->
    (ids (F, H, W) uint8, centres (F, K, 2) int32 (y, x), n (F,) int32, capped (F,) int32) on the device.  Nothing is read back."""
    assert center.dtype == torch.float32 and center.dim() == 3, 'bev_instance_decode: centre maps (F, H, W) float32'
    F, H, W = (int(v) for v in center.shape)
    assert offset.dtype == torch.float32 and tuple(offset.shape) == (F, 2, H, W), 'bev_instance_decode: offsets (F, 2, H, W) float32'
    assert (logits is None) != (foreground is None), 'bev_instance_decode: either logits or a foreground mask'
    K, radius = int(max_centres), int(radius)
    if not 1 <= K <= 254:
        raise ValueError(f'bev_instance_decode: {K} centres outside 1..254')
    if not 1 <= radius <= 3:
        raise ValueError(f'bev_instance_decode: radius {radius} outside 1..3')
    if math.isnan(float(threshold)):
        raise ValueError('bev_instance_decode: the threshold is NaN')
    Cn, things = 0, 0
    if logits is not None:
        assert logits.dtype == torch.float32 and logits.dim() == 4 and (logits.shape[0], *logits.shape[2:]) == (F, H, W), \
            'bev_instance_decode: logits (F, C, H, W) float32'
        Cn = int(logits.shape[1])
        if not 2 <= Cn <= 32:
            raise ValueError(f'bev_instance_decode: {Cn} classes outside 2..32')
        for k in thing_classes:
            if not 0 <= int(k) < 32:
                raise ValueError(f'bev_instance_decode: thing class {k} outside 0..31')
            things |= 1 << int(k)
    else:
        assert foreground.dtype == torch.uint8 and tuple(foreground.shape) == (F, H, W), 'bev_instance_decode: foreground mask (F, H, W) uint8'
    src = logits if logits is not None else foreground
    assert offset.device == center.device and src.device == center.device, 'bev_instance_decode: tensors of one device'
    nbytes = int(lib().muvo_bev_instance_ws_bytes(_i64(F), H, W))
    if nbytes < 0:
        raise ValueError(f'bev_instance_decode: {F} frames of {H} x {W} (1..65535 frames, 1..4096 a side, at most 2^24 pixels)')
    center, offset, src = center.contiguous(), offset.contiguous(), src.contiguous()
    dev = center.device
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.int64)
    ids = torch.empty((F, H, W), device=dev, dtype=torch.uint8)
    centres = torch.empty((F, K, 2), device=dev, dtype=torch.int32)
    n = torch.empty((F,), device=dev, dtype=torch.int32)
    capped = torch.empty((F,), device=dev, dtype=torch.int32)
    _ck(lib().muvo_bev_instance_decode(_f(center), _f(offset), _f(src) if logits is not None else None, Cn, C.c_uint32(things),
                                       _p(src) if logits is None else None, _i64(F), H, W, _fl(threshold), radius, K, _p(ws), _i64(nbytes), _p(ids),
                                       _p(centres), _p(n), _p(capped), _st()))
    return ids, centres, n, capped


def bev_pq_counts(label, pred, counts, iou_sum, capped=None):
    """counts (7,) int64 - frames, capped frames, label segments, predicted segments, tp, fp, fn - and iou_sum (1,) float64 on the
    device are added to, over the F frames of the id maps label and pred (F, H, W) uint8, 0 = none (include/muvo_hip.h:
    muvo_bev_pq_counts); capped: the (F,) int32 flags of bev_instance_decode, or None.  Nothing is read back."""
    for t in (label, pred):
        assert t.dtype == torch.uint8 and t.dim() == 3, 'bev_pq_counts: id maps (F, H, W) uint8'
    assert label.shape == pred.shape and label.device == pred.device, 'bev_pq_counts: label and prediction of one shape'
    F, H, W = (int(v) for v in label.shape)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (7,) and counts.is_contiguous() and counts.device == label.device, \
        'bev_pq_counts: counts (7,) int64'
    assert iou_sum.dtype == torch.float64 and tuple(iou_sum.shape) == (1,) and iou_sum.is_contiguous() and iou_sum.device == label.device, \
        'bev_pq_counts: iou_sum (1,) float64'
    if capped is not None:
        assert capped.dtype == torch.int32 and tuple(capped.shape) == (F,) and capped.device == label.device, 'bev_pq_counts: capped (F,) int32'
        capped = capped.contiguous()
    nbytes = int(lib().muvo_bev_pq_ws_bytes(_i64(F)))
    if nbytes < 0 or not (1 <= H <= 4096 and 1 <= W <= 4096 and H * W <= 1 << 24):
        raise ValueError(f'bev_pq_counts: {F} frames of {H} x {W} (1..65535 frames, 1..4096 a side, at most 2^24 pixels)')
    label, pred = label.contiguous(), pred.contiguous()
    ws = torch.empty(nbytes // 8, device=label.device, dtype=torch.int64)
    _ck(lib().muvo_bev_pq_counts(_p(label), _p(pred), _p(capped), _i64(F), H, W, _p(counts), _p(iou_sum), _p(ws), _i64(nbytes), _st()))


# ---- calibration and uncertainty of a sample ensemble (csrc/calibration.hip; include/muvo_hip.h: muvo_voxel_calibration) -----------
CALIBRATION_MAX_SAMPLES, CALIBRATION_MAX_CLASSES, CALIBRATION_MAX_BINS = 8, 16, 32
CALIBRATION_FIX = float(1 << 24)          # the unit of the fixed-point words: real sum = word / CALIBRATION_FIX


def voxel_calibration(logits_list, label, table, counts, ssc, sums, ens=None, top_entropy=None, top_mi=None):
    """The K tensors of logits_list, (F, C, X, Y, Z) float32 each, against label (F, X, Y, Z) uint8 (255 = ignore): table (B, 3) int64,
    counts (4,) int64, ssc (3 + 3 C,) int64 and sums (6,) int64 on the device are added to; ens (F, X, Y, Z) uint8 and top_entropy,
    top_mi (F, X, Y) uint8 are written when given (include/muvo_hip.h: muvo_voxel_calibration).  Nothing is read back."""
    logits_list = list(logits_list)
    K = len(logits_list)
    if not 1 <= K <= CALIBRATION_MAX_SAMPLES:
        raise ValueError(f'voxel_calibration: {K} samples (1..{CALIBRATION_MAX_SAMPLES})')
    first = logits_list[0]
    assert first.dim() == 5 and first.dtype == torch.float32, 'voxel_calibration: logits (F, C, X, Y, Z) float32'
    F, Cn, X, Y, Z = (int(v) for v in first.shape)
    dev = first.device
    for t in logits_list:
        assert t.dtype == torch.float32 and t.shape == first.shape and t.device == dev, 'voxel_calibration: samples of one shape, dtype and device'
    assert label.dtype == torch.uint8 and tuple(label.shape) == (F, X, Y, Z) and label.device == dev, 'voxel_calibration: label (F, X, Y, Z) uint8'
    if not 2 <= Cn <= CALIBRATION_MAX_CLASSES:
        raise ValueError(f'voxel_calibration: {Cn} classes (2..{CALIBRATION_MAX_CLASSES})')
    assert table.dim() == 2 and table.shape[1] == 3, 'voxel_calibration: table (B, 3) int64'
    B = int(table.shape[0])
    if not 1 <= B <= CALIBRATION_MAX_BINS:
        raise ValueError(f'voxel_calibration: {B} bins (1..{CALIBRATION_MAX_BINS})')
    if F < 1 or min(X, Y, Z) < 1 or F * X * Y * Z > 1 << 40:
        raise ValueError(f'voxel_calibration: {F} frames of {X} x {Y} x {Z} (at least one voxel, at most 2^40)')
    for t, shape, what in ((table, (B, 3), 'table (B, 3)'), (counts, (4,), 'counts (4,)'), (ssc, (3 + 3 * Cn,), 'ssc (3 + 3 C,)'), (sums, (6,), 'sums (6,)')):
        assert t.dtype == torch.int64 and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev, f'voxel_calibration: {what} int64'
    for t, shape, what in ((ens, (F, X, Y, Z), 'ens (F, X, Y, Z)'), (top_entropy, (F, X, Y), 'top_entropy (F, X, Y)'), (top_mi, (F, X, Y), 'top_mi (F, X, Y)')):
        assert t is None or (t.dtype == torch.uint8 and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev), f'voxel_calibration: {what} uint8'
    logits_list = [t.contiguous() for t in logits_list]
    label = label.contiguous()
    ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in logits_list])
    for t in logits_list:
        _f(t)
    _ck(lib().muvo_voxel_calibration(ptrs, K, _p(label), _i64(F), Cn, X, Y, Z, B, _p(table), _p(counts), _p(ssc), _p(sums), _p(ens), _p(top_entropy),
                                     _p(top_mi), _st()))


# ================================================================================================ ICP between lidar frames
ICP_RUNNING, ICP_CONVERGED, ICP_MAX_ITERATION, ICP_FEW_INLIERS, ICP_EMPTY, ICP_BAD_FRAME = 0, 1, 2, 3, 4, 5
ICP_CHUNK = 8                      # iterations queued between two looks at the `done` words
IcpResult = collections.namedtuple('IcpResult', 'T fitness inlier_rmse iterations converged status')


def _icp_setup(src, tgt, src_frames, tgt_frames, scale, threshold, init, source_stride):
    assert src.dim() == 3 and tgt.dim() == 3 and src.shape[2] == tgt.shape[2], 'icp: planar (F, C, n) tensors of one n'
    assert src.shape[1] >= 4 and tgt.shape[1] >= 4, 'icp: x, y, z, range are planes 0..3'
    assert src.device == tgt.device
    if src.dtype != torch.float32 or tgt.dtype != torch.float32:
        raise ValueError(f'icp: float32 tensors, got {src.dtype} and {tgt.dtype}')
    if int(source_stride) < 1 or int(source_stride) > src.shape[2]:
        raise ValueError(f'icp: source_stride {source_stride} outside [1, n]')
    if not (float(scale) > 0 and float(threshold) > 0):
        raise ValueError(f'icp: scale {scale} and threshold {threshold} must be positive')
    dev, n = src.device, src.shape[2]
    sf = [int(v) for v in (src_frames.tolist() if torch.is_tensor(src_frames) else src_frames)]
    tf = [int(v) for v in (tgt_frames.tolist() if torch.is_tensor(tgt_frames) else tgt_frames)]
    if len(sf) != len(tf) or not sf:
        raise ValueError('icp: src_frames and tgt_frames must be two non-empty lists of one length')
    if min(sf) < 0 or max(sf) >= src.shape[0] or min(tf) < 0 or max(tf) >= tgt.shape[0]:
        raise ValueError('icp: a frame index outside its tensor')
    P, L = len(sf), lib()
    frames = torch.tensor([sf, tf], dtype=torch.int32).to(dev)
    state = torch.empty(P, int(L.muvo_icp_state_doubles()), device=dev, dtype=torch.float64)
    done = torch.empty(P, device=dev, dtype=torch.int32)
    ws = torch.empty(max(1, L.muvo_icp_ws_doubles(_i64(P), _i64(n), _i64(source_stride))), device=dev, dtype=torch.float64)
    if init is not None:
        init = torch.as_tensor(init, dtype=torch.float64).reshape(P, 4, 4)[:, :3].contiguous().to(dev)
    _ck(L.muvo_icp_init(_f(src), _f(tgt), _i64(src.shape[0]), _i64(tgt.shape[0]), int(src.shape[1]), int(tgt.shape[1]), _i64(n),
                        _p(frames[0]), _p(frames[1]), _i64(P), _i64(source_stride), _p(init), _p(state), _p(done), _st()))
    return frames, state, done, ws, P, n


ICP_SEARCHES = ('brute', 'grid')


def _icp_search(search):
    """refuses an unknown search before the library is loaded or a device is touched"""
    if search not in ICP_SEARCHES:
        raise ValueError(f"icp: search must be 'brute' or 'grid', got {search!r}")
    return search


def _icp_grid(tgt, frames, P, n, scale, threshold, done):
    """search='grid': the cell grid of every pair's target points (muvo_icp_grid_build), built once per call after
    muvo_icp_init on the current stream, no host read; a byte tensor owned by the call"""
    L = lib()
    grid = torch.empty(max(16, int(L.muvo_icp_grid_bytes(_i64(P), _i64(n)))), device=tgt.device, dtype=torch.uint8)
    _ck(L.muvo_icp_grid_build(_f(tgt), int(tgt.shape[1]), _i64(n), _p(frames[1]), _i64(P), _fl(scale), _fl(threshold), _p(done), _p(grid),
                              _i64(grid.numel()), _st()))
    return grid


def _icp_iterate(src, tgt, frames, P, n, scale, threshold, stride, max_iteration, count, ws, state, done, corr=None, sums=None, grid=None):
    if grid is not None:
        _ck(lib().muvo_icp_iterate_grid(_f(src), _f(tgt), int(src.shape[1]), int(tgt.shape[1]), _i64(n), _p(frames[0]), _p(frames[1]),
                                        _i64(P), _fl(scale), _fl(threshold), _i64(stride), int(max_iteration), int(count), _p(ws),
                                        _p(state), _p(done), _p(corr), _p(sums), _p(grid), _i64(grid.numel()), _st()))
        return
    _ck(lib().muvo_icp_iterate(_f(src), _f(tgt), int(src.shape[1]), int(tgt.shape[1]), _i64(n), _p(frames[0]), _p(frames[1]), _i64(P),
                               _fl(scale), _fl(threshold), _i64(stride), int(max_iteration), int(count), _p(ws), _p(state), _p(done),
                               _p(corr), _p(sums), _st()))


def _icp_result(state):
    T = torch.zeros(state.shape[0], 4, 4, dtype=torch.float64, device=state.device)
    T[:, :3] = state[:, :12].view(-1, 3, 4)
    T[:, 3, 3] = 1.0
    status = state[:, 18].long()
    return IcpResult(T, state[:, 12].clone(), state[:, 13].clone(), state[:, 17].long(), status == ICP_CONVERGED, status)


def _search_keyword(fn):
    """icp_register keeps the parameter list its callers pin by introspection and takes one more keyword, `search`: 'brute' runs
    the function as it always was, 'grid' the same registration over the cell grid; anything else is refused before the library is
    loaded or a device is touched."""
    @functools.wraps(fn)
    def call(*args, search='brute', **kw):
        if _icp_search(search) == 'brute':
            return fn(*args, **kw)
        return _icp_run(*args, search=search, **kw)
    return call


@_search_keyword
def icp_register(src, tgt, src_frames, tgt_frames, scale, threshold, max_iteration=2000, init=None, source_stride=1):
    """Point-to-point ICP (include/muvo_hip.h: muvo_icp_*) of P frame pairs: pair p moves frame src_frames[p] of src (F, C, n)
    onto frame tgt_frames[p] of tgt (the same tensor twice is fine: no copy).  Planes 0..2 = x, y, z (times `scale`), plane 3 =
    range, valid iff range > 0.  Returns IcpResult of device tensors: T (P, 4, 4) float64 (target ~ T [source; 1]), fitness,
    inlier_rmse (P,) float64, iterations (P,) int64, converged (P,) bool (stopped by the 1e-6 deltas) and status (ICP_*).
    The host queues ICP_CHUNK iterations at a time and then reads the P done words: no sync per iteration.  init: (P, 4, 4)
    start poses (default identity); source_stride k: only source points 0, k, 2k ... are queries (cost knob, 1 = exact).
    Keyword search='brute' (every query scans every target point) or 'grid' (a cell grid of the target points, built once per
    call; the same result bit for bit, see muvo_icp_iterate_grid)."""
    return _icp_run(src, tgt, src_frames, tgt_frames, scale, threshold, max_iteration, init, source_stride)


def icp_register_queued(src, tgt, src_frames, tgt_frames, scale, threshold, max_iteration, init=None, source_stride=1, search='brute'):
    """icp_register for a caller that must not wait for the device: all max_iteration + 1 evaluations are queued and the `done`
    words are never read (a pair that has stopped costs workgroups that return at once).  The same IcpResult, bit for bit: what a
    pair computes does not depend on when the host looks.  For small budgets - the cost is max_iteration + 1 launches whatever
    the clouds are."""
    return _icp_run(src, tgt, src_frames, tgt_frames, scale, threshold, max_iteration, init, source_stride, read_done=False, search=search)


def _icp_run(src, tgt, src_frames, tgt_frames, scale, threshold, max_iteration=2000, init=None, source_stride=1, on_chunk=None, read_done=True,
             search='brute'):
    """icp_register; on_chunk(state, done) is called after every chunk (tests look at the state between chunks)"""
    _icp_search(search)
    if int(max_iteration) < 0:
        raise ValueError(f'icp: max_iteration {max_iteration} is negative')
    src, tgt = src.contiguous(), tgt.contiguous()
    frames, state, done, ws, P, n = _icp_setup(src, tgt, src_frames, tgt_frames, scale, threshold, init, source_stride)
    grid = _icp_grid(tgt, frames, P, n, scale, threshold, done) if search == 'grid' else None
    queued = 0
    while queued < max_iteration + 1:             # max_iteration fits need max_iteration + 1 evaluations
        count = min(ICP_CHUNK, max_iteration + 1 - queued)
        _icp_iterate(src, tgt, frames, P, n, scale, threshold, source_stride, max_iteration, count, ws, state, done, grid=grid)
        queued += count
        if on_chunk is not None:
            on_chunk(state, done)
        if read_done and bool(done.cpu().all()):
            break
    return _icp_result(state)


def icp_step(src, tgt, src_frames, tgt_frames, scale, threshold, init=None, source_stride=1, out=None, search='brute'):
    """One evaluation at `init` (default identity) and the fit that follows it: (corr (P, n) int32 - the target index of every
    source point, -1 = invalid, gated out or no query -, sums (P, 17) float64 over the inliers - count, sum d^2, sum s, sum q,
    sum s q^T -, IcpResult after the step).  Pairs that are empty report zeros and -1.  out = (corr, sums): contiguous device
    tensors of those shapes and types to write into (they are initialised here).  search: as icp_register."""
    _icp_search(search)
    src, tgt = src.contiguous(), tgt.contiguous()
    frames, state, done, ws, P, n = _icp_setup(src, tgt, src_frames, tgt_frames, scale, threshold, init, source_stride)
    if out is None:
        out = (torch.empty((P, n), device=src.device, dtype=torch.int32), torch.empty(P, 17, device=src.device, dtype=torch.float64))
    corr, sums = out
    if (corr.shape, corr.dtype, sums.shape, sums.dtype) != ((P, n), torch.int32, (P, 17), torch.float64):
        raise ValueError(f'icp_step: out must be ({P}, {n}) int32 and ({P}, 17) float64')
    corr.fill_(-1)
    sums.zero_()
    grid = _icp_grid(tgt, frames, P, n, scale, threshold, done) if search == 'grid' else None
    _icp_iterate(src, tgt, frames, P, n, scale, threshold, source_stride, 2000, 1, ws, state, done, corr, sums, grid=grid)
    return corr, sums, _icp_result(state)


# ================================================================================================ optical flow between camera frames
FLOW_WORKSPACE_CAP = 512 << 20     # bytes of workspace a call may hold: the pairs run in chunks below it (at least one pair)


def _flow_indices(v, what):
    v = [int(i) for i in (v.tolist() if torch.is_tensor(v) else v)]
    if not v:
        raise ValueError(f'optical_flow: {what} is empty')
    return v


def optical_flow(frames_a, frames_b, pairs_a, pairs_b, out=None):
    """Dense Farneback flow (include/muvo_hip.h: muvo_flow_farneback, our definition) of P frame pairs: pair p goes from frame
    pairs_a[p] of frames_a (Fa, 3, h, w) float32 to frame pairs_b[p] of frames_b (the same tensor twice is fine: no frame is
    copied); index -1 is an all-white frame.  Returns (P, 2, h, w) float32 [dx, dy] on the device.  The pairs run in chunks of at
    most muvo_flow_max_pairs() whose workspace stays below FLOW_WORKSPACE_CAP; the workspace is kept between calls."""
    if frames_a.dtype != torch.float32 or frames_b.dtype != torch.float32:
        raise ValueError(f'optical_flow: float32 frames, got {frames_a.dtype} and {frames_b.dtype}')
    if frames_a.dim() != 4 or frames_b.dim() != 4 or frames_a.shape[1] != 3 or frames_a.shape[1:] != frames_b.shape[1:]:
        raise ValueError(f'optical_flow: two stacks (F, 3, h, w) of one frame size, got {tuple(frames_a.shape)} and {tuple(frames_b.shape)}')
    assert frames_a.device == frames_b.device
    frames_a, frames_b = frames_a.contiguous(), frames_b.contiguous()
    pa, pb = _flow_indices(pairs_a, 'pairs_a'), _flow_indices(pairs_b, 'pairs_b')
    if len(pa) != len(pb):
        raise ValueError('optical_flow: pairs_a and pairs_b must have one length')
    L, P, (h, w) = lib(), len(pa), frames_a.shape[2:]
    one = int(L.muvo_flow_workspace_bytes(_i64(1), int(h), int(w)))
    if one < 0:
        raise ValueError(f'optical_flow: frames of {h} x {w} (16..8192 on both axes)')
    chunk = max(1, min(int(L.muvo_flow_max_pairs()), FLOW_WORKSPACE_CAP // one, P))
    ws = scratch('optical_flow', (chunk * one + 3) // 4, frames_a.device)
    flow = out if out is not None else torch.empty((P, 2, h, w), dtype=torch.float32, device=frames_a.device)
    assert flow.shape == (P, 2, h, w) and flow.dtype == torch.float32 and flow.is_contiguous()
    for at in range(0, P, chunk):
        n = min(chunk, P - at)
        ia, ib = (C.c_int32 * n)(*pa[at:at + n]), (C.c_int32 * n)(*pb[at:at + n])
        _ck(L.muvo_flow_farneback(_f(frames_a), _i64(frames_a.shape[0]), _f(frames_b), _i64(frames_b.shape[0]), int(h), int(w), ia, ib, _i64(n),
                                  _p(ws), _i64(ws.numel() * 4), _f(flow[at:at + n]), _st()))
    return flow


def flow_colour(flow, panel, place, pad=5, padbyte=204):
    """Colour-coded tiles (include/muvo_hip.h: muvo_flow_colour) of P flow fields (P, 2, h, w) float32 in a 3-channel panel."""
    assert flow.dtype == torch.float32 and flow.dim() == 4 and flow.shape[1] == 2 and flow.is_contiguous()
    assert panel.dim() == 4 and panel.shape[1] == 3
    P, _, h, w = flow.shape
    ws = scratch('flow_colour', max(1, lib().muvo_flow_colour_ws_bytes(_i64(P)) // 4), flow.device)
    _ck(lib().muvo_flow_colour(_f(flow), _i64(P), int(h), int(w), _p(ws), _i64(ws.numel() * 4), int(pad), int(padbyte), *_panel_args(panel, place)))


def flow_epe(flow_a, flow_b, acc):
    """acc (3,) float64 on the device += (sum |a - b|, sum |a|, pixels) over the pixels at least 5 from the border of the P pairs
    of flow fields (P, 2, h, w) float32 (include/muvo_hip.h: muvo_flow_epe); nothing is read back."""
    assert flow_a.shape == flow_b.shape and flow_a.dtype == flow_b.dtype == torch.float32 and flow_a.is_contiguous() and flow_b.is_contiguous()
    assert acc.dtype == torch.float64 and acc.numel() == 3 and acc.is_contiguous()
    P, _, h, w = flow_a.shape
    ws = scratch('flow_epe', max(1, lib().muvo_flow_epe_ws_doubles(_i64(P))), flow_a.device, torch.float64)
    _ck(lib().muvo_flow_epe(_f(flow_a), _f(flow_b), _i64(P), int(h), int(w), _p(ws), _i64(ws.numel()), _p(acc), _st()))



# ================================================================================================ optimiser
def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    _ck(lib().muvo_adamw_step(_f(p), _f(g), _f(m), _f(v), _i64(p.numel()), _fl(lr), _fl(beta1), _fl(beta2), _fl(eps),
                              _fl(weight_decay), int(step), _fl(grad_scale), _st()))


# ================================================================================================ time stack / unstack
class StackTimeFn(torch.autograd.Function):
    """list of s tensors (b, D) -> (b, s, D) via strided 2-D copies."""

    @staticmethod
    def forward(ctx, *xs):
        s = len(xs)
        b, d = xs[0].shape
        y = torch.empty(b, s, d, device=xs[0].device, dtype=torch.float32)
        for t, x in enumerate(xs):
            x = x.contiguous()
            _ck(lib().muvo_copy2d(_f(x), C.c_void_p(y.data_ptr() + 4 * t * d), _i64(b), _i64(d), _i64(d), _i64(s * d), 0,
                                  _st()))
        ctx.dims = (b, s, d)
        return y

    @staticmethod
    def backward(ctx, dy):
        b, s, d = ctx.dims
        dy = dy.contiguous()
        outs = []
        for t in range(s):
            if ctx.needs_input_grad[t]:
                g = torch.empty(b, d, device=dy.device, dtype=torch.float32)
                _ck(lib().muvo_copy2d(C.c_void_p(dy.data_ptr() + 4 * t * d), _f(g), _i64(b), _i64(d), _i64(s * d), _i64(d),
                                      0, _st()))
                outs.append(g)
            else:
                outs.append(None)
        return tuple(outs)


def stack_time(xs):
    return StackTimeFn.apply(*xs)


class UnstackTimeFn(torch.autograd.Function):
    """(b, s, D) -> tuple of s contiguous (b, D) tensors."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        b, s, d = x.shape
        outs = []
        for t in range(s):
            g = torch.empty(b, d, device=x.device, dtype=torch.float32)
            _ck(lib().muvo_copy2d(C.c_void_p(x.data_ptr() + 4 * t * d), _f(g), _i64(b), _i64(d), _i64(s * d), _i64(d), 0,
                                  _st()))
            outs.append(g)
        ctx.dims = (b, s, d)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        b, s, d = ctx.dims
        dev = next(g.device for g in gs if g is not None)
        dx = torch.zeros(b, s, d, device=dev, dtype=torch.float32)
        for t, g in enumerate(gs):
            if g is None:
                continue
            g = g.contiguous()
            _ck(lib().muvo_copy2d(_f(g), C.c_void_p(dx.data_ptr() + 4 * t * d), _i64(b), _i64(d), _i64(d), _i64(s * d), 0,
                                  _st()))
        return dx


def unstack_time(x):
    return UnstackTimeFn.apply(x)


class SegmentMarkFn(torch.autograd.Function):
    """Identity whose backward calls `cb(name)` first: placed on the input of a sub-network it tells the data-parallel
    reducer that backward has issued every kernel of that sub-network (muvo_amd/parallel.py)."""

    @staticmethod
    def forward(ctx, x, cb, name):
        ctx.cb, ctx.name = cb, name
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.cb(ctx.name)
        return g, None, None


def segment_mark(x, cb, name):
    return SegmentMarkFn.apply(x, cb, name)


class SumScalarsFn(torch.autograd.Function):
    """total = sum of 0-d tensors (trainer.py:511-513 loss_reducing)."""

    @staticmethod
    def forward(ctx, *vals):
        out = torch.zeros(1, device=vals[0].device, dtype=torch.float32)
        for v in vals:
            _ck(lib().muvo_copy2d(C.c_void_p(v.data_ptr()), _f(out), _i64(1), _i64(1), _i64(1), _i64(1), 1, _st()))
        ctx.n = len(vals)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        return tuple(g for _ in range(ctx.n))


def sum_scalars(vals):
    return SumScalarsFn.apply(*vals)


# ------------------------------------------------------------------------------------------------
# one-GPU stand-in for a gradient all-reduce among `peers` GPUs (include/muvo_hip.h: muvo_fake_allreduce)
_FAKE_AR = {}


def fake_allreduce(buf, peers=8, workgroups=None, ms_per_100mb=None):
    """Runs on the current stream; leaves buf bit-identical.  Rate: 1 ms per 100 MB (an 8-GPU xGMI ring at ~175 GB/s of bus
    bandwidth: 2 (G-1)/G x 100 MB / 175 GB/s; RCCL reaches more on large messages, so this is the pessimistic side;
    MUVO_DP_FAKE_MS_PER_100MB overrides).  The sleep count that gives this rate with
    `workgroups` resident workgroups (RCCL-like: MUVO_DP_FAKE_WGS, default 32) is calibrated once per device on a scratch buffer."""
    dev = buf.device
    wgs = int(workgroups or os.environ.get('MUVO_DP_FAKE_WGS', '32'))
    target = float(ms_per_100mb or os.environ.get('MUVO_DP_FAKE_MS_PER_100MB', '1.0'))
    key = (dev.index, wgs, round(target, 4))
    sleep = _FAKE_AR.get(key)
    L = lib()
    if sleep is None:
        probe = torch.zeros(16 * 2 ** 20, device=dev, dtype=torch.float32)        # 64 MB
        ms = {}
        for sl in (0, 64):
            for _ in range(2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _ck(L.muvo_fake_allreduce(_f(probe), _i64(probe.numel()), wgs, sl, _st()))
                e1.record()
                e1.synchronize()
                ms[sl] = e0.elapsed_time(e1) * 100.0 / 64.0            # per 100 MB
        per = max((ms[64] - ms[0]) / 64.0, 1e-6)
        sleep = int(max(0, round((target - ms[0]) / per)))
        _FAKE_AR[key] = sleep
        _FAKE_AR[('calibration',) + key] = dict(ms_per_100mb_sleep0=ms[0], ms_per_100mb_sleep64=ms[64], sleep=sleep, target=target, workgroups=wgs)
    n = buf.numel() & ~3
    if n:
        _ck(L.muvo_fake_allreduce(_f(buf), _i64(n), wgs, sleep, _st()))


def fake_allreduce_calibration():
    return [v for k, v in _FAKE_AR.items() if k and k[0] == 'calibration']


# ---- prediction export (csrc/export.hip) -----------------------------------------------------------------------------------------
VOXEL_ROWS_CHUNK = 2048        # EXP_CHUNK of csrc/export.hip: voxels per workgroup of the counting and the compaction pass


def _voxel_rows_args(src):
    """(contiguous source, is_logits, F, C, X, Y, Z, scratch) of a voxel_rows call."""
    if src.dtype == torch.float32 and src.dim() == 5:
        F, Cn, X, Y, Z = src.shape
        logits = True
    elif src.dtype == torch.uint8 and src.dim() == 4:
        (F, X, Y, Z), Cn, logits = src.shape, 0, False
    else:
        raise ValueError(f'voxel_rows: class logits (F, C, X, Y, Z) float32 or a class grid (F, X, Y, Z) uint8, got '
                         f'{tuple(src.shape)} {src.dtype}')
    nbytes = lib().muvo_voxel_rows_scratch_bytes(int(F), int(X), int(Y), int(Z))
    if nbytes < 0:
        raise RuntimeError(f'voxel_rows: sizes F {F}, grid {X} {Y} {Z} are not supported (include/muvo_hip.h)')
    return src.contiguous(), logits, int(F), int(Cn), int(X), int(Y), int(Z), scratch('voxel_rows', nbytes, src.device, torch.uint8)


def _voxel_rows_call(src, logits, F, Cn, X, Y, Z, ws, rows, cap, counts):
    L = lib()
    if logits:
        _ck(L.muvo_voxel_rows_logits(_f(src), F, Cn, X, Y, Z, _p(ws), _p(rows), _i64(cap), _p(counts), _st()))
    else:
        _ck(L.muvo_voxel_rows_grid(_p(src), F, X, Y, Z, _p(ws), _p(rows), _i64(cap), _p(counts), _st()))


def voxel_rows_into(src, rows, cap=None):
    """One call of the entry point with a caller-owned buffer: `rows` (>= cap, 4) uint16 receives the first `cap` (default: all of
    the buffer) rows, the returned counts (F,) int64 are the true totals whatever the capacity.  No host synchronisation."""
    assert rows.dtype == torch.uint16 and rows.dim() == 2 and rows.shape[1] == 4 and rows.is_contiguous()
    cap = rows.shape[0] if cap is None else int(cap)
    assert 0 <= cap <= rows.shape[0]
    src, logits, F, Cn, X, Y, Z, ws = _voxel_rows_args(src)
    counts = torch.empty(F, dtype=torch.int64, device=src.device)
    _voxel_rows_call(src, logits, F, Cn, X, Y, Z, ws, rows if cap else None, cap, counts)
    return counts


def voxel_rows(src):
    """Occupied-voxel rows of F frames: src = class logits (F, C, X, Y, Z) float32 (class = torch.argmax over C) or a class grid
    (F, X, Y, Z) uint8.  Returns (rows (Q, 4) uint16 device tensor: x, y, z, class of every voxel whose class is not 0, in the
    order of torch.where, frames concatenated; counts: F Python ints).  The counting pass runs first, the host reads the F
    counts (the one synchronisation of the call), the rows are then written into a tensor of exactly their size - the logits are
    read once, the byte grid between the passes stays on the device."""
    src, logits, F, Cn, X, Y, Z, ws = _voxel_rows_args(src)
    counts = torch.empty(F, dtype=torch.int64, device=src.device)
    _voxel_rows_call(src, logits, F, Cn, X, Y, Z, ws, None, 0, counts)
    per_frame = counts.tolist()
    total = sum(per_frame)
    rows = torch.empty((total, 4), dtype=torch.uint16, device=src.device)
    if total:
        _ck(lib().muvo_voxel_rows_write(_p(None if logits else src), F, X, Y, Z, _p(ws), _p(counts), _p(rows), _i64(total), _st()))
    return rows, per_frame


def image_u8(x):
    """float32 tensor (any shape; made contiguous) -> uint8 of the same shape: trunc(x * 255) SATURATED to [0, 255], NaN -> 0.
    Equal to numpy's `(x * 255).astype(np.uint8)` wherever that is defined (0 <= x * 255 < 256); outside it - the decoder heads
    have no squashing activation - the cast of the reference is implementation-defined and this is the product's definition."""
    assert x.dtype == torch.float32
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if x.numel():
        _ck(lib().muvo_image_u8(_f(x), _p(y), _i64(x.numel()), _st()))
    return y


# ---- prediction panels (csrc/visualise.hip) --------------------------------------------------------------------------------------
class TilePlace(C.Structure):
    """MuvoTilePlace of include/muvo_hip.h: where the tiles of one call go inside the panel."""
    _fields_ = [('sample_stride', C.c_int64), ('chan_stride', C.c_int64), ('PH', C.c_int32), ('PW', C.c_int32),
                ('T', C.c_int32), ('t0', C.c_int32), ('x0', C.c_int32), ('y0', C.c_int32), ('xstep', C.c_int32), ('ystep', C.c_int32),
                ('tsep', C.c_int32), ('sepw', C.c_int32)]


PANEL_NO_SEP = 1 << 30          # tsep of a layout without a separator


def tile_place(panel, T, t0=0, x0=0, y0=0, xstep=0, ystep=0, tsep=PANEL_NO_SEP, sepw=0):
    """The placement of T tiles per sample in `panel`: (b, C, PH, PW) uint8, or a video (b, Tv, 1, H2, W), whose frames are
    addressed as one (Tv * H2) x W plane per sample.  Step t = t0 + frame % T starts at row y0 + t * ystep, column
    x0 + t * xstep (+ sepw when t >= tsep)."""
    assert panel.dtype == torch.uint8 and panel.is_cuda and panel.is_contiguous() and panel.dim() in (4, 5)
    if panel.dim() == 5:
        b, Tv, ch, H2, W = panel.shape
        assert ch == 1
        PH, PW, cs = Tv * H2, W, Tv * H2 * W
        ss = cs
    else:
        b, ch, PH, PW = panel.shape
        cs, ss = PH * PW, ch * PH * PW
    return TilePlace(ss, cs, PH, PW, int(T), int(t0), int(x0), int(y0), int(xstep), int(ystep), int(tsep), int(sepw))


def _panel_args(panel, place):
    assert panel.dtype == torch.uint8 and panel.is_contiguous()
    return _p(panel), _i64(panel.numel()), C.byref(place), _st()


def _panel_nch(panel):
    return 1 if panel.dim() == 5 else int(panel.shape[1])


def _palette(palette, device):
    assert palette.dtype == torch.uint8 and tuple(palette.shape) == (256, 3) and palette.device == device
    return _p(palette)


def panel_image(src, panel, place, pad=0, padbyte=0, channel=0):
    """Float image tiles: the panel's 1 or 3 channels are channels `channel` ... of src (F, C, h, w) float32 (a negative
    `channel` counts from the end); bytes by the rule of image_u8."""
    assert src.dtype == torch.float32 and src.dim() == 4
    src = src.contiguous()
    F, Cn, h, w = src.shape
    c0 = channel + Cn if channel < 0 else channel
    _ck(lib().muvo_panel_image(_f(src), int(F), int(Cn), int(c0), int(h), int(w), int(pad), int(padbyte), _panel_nch(panel),
                               *_panel_args(panel, place)))


def panel_classes(src, palette, panel, place, pad=0, padbyte=0, rotate=False):
    """Class tiles: src = logits (F, C, h, w) float32 (first maximum over C, strict >) or labels (F, h, w) uint8 / int64;
    palette (256, 3) uint8 on the device.  rotate: the padded tile goes in as torch.rot90(k=1)."""
    src = src.contiguous()
    pal = _palette(palette, src.device)
    if src.dtype == torch.float32 and src.dim() == 4:
        F, Cn, h, w = src.shape
        _ck(lib().muvo_panel_logits(_f(src), int(F), int(Cn), int(h), int(w), pal, int(pad), int(padbyte), int(bool(rotate)),
                                    *_panel_args(panel, place)))
    elif src.dtype in (torch.uint8, torch.int64) and src.dim() == 3:
        F, h, w = src.shape
        _ck(lib().muvo_panel_labels(_p(src), int(src.dtype == torch.int64), int(F), int(h), int(w), pal, int(pad), int(padbyte),
                                    int(bool(rotate)), *_panel_args(panel, place)))
    else:
        raise ValueError(f'panel_classes: logits (F, C, h, w) float32 or labels (F, h, w) uint8 / int64, got {tuple(src.shape)} {src.dtype}')


def panel_fill(F, h, w, value, panel, place, pad=0, padbyte=0):
    """Constant tiles: h x w of `value` inside a border of `padbyte`, F of them."""
    _ck(lib().muvo_panel_fill(int(F), int(h), int(w), int(value), int(pad), int(padbyte), _panel_nch(panel), *_panel_args(panel, place)))


def panel_bars(values, kind, h, w, panel, place):
    """Action bars of an h x w camera image: values (F,) float32 on the device (never read by the host); kind 0
    throttle_brake, 1 steering.  A tile is (int(h / 4), w + 10)."""
    assert values.dtype == torch.float32
    values = values.contiguous().view(-1)
    _ck(lib().muvo_panel_bars(_f(values), int(kind), int(values.numel()), int(h), int(w), *_panel_args(panel, place)))


def panel_scatter(range_view, scale, panel, place, pad=0, padbyte=0):
    """Bird's-eye scatter of range views (F, C, H, W) float32 (x, y, ..., range) on 256 x 256 tiles (pcd_xy_image)."""
    assert range_view.dtype == torch.float32 and range_view.dim() == 4
    range_view = range_view.contiguous()
    F, Cn, H, W = range_view.shape
    _ck(lib().muvo_panel_scatter(_f(range_view), int(F), int(Cn), int(H), int(W), _fl(scale), int(pad), int(padbyte),
                                 *_panel_args(panel, place)))


def panel_voxel_top(src, palette, panel, place, pad=0, padbyte=0):
    """Top view of voxel grids: src = logits (F, C, X, Y, Z) float32 or a class grid (F, X, Y, Z) uint8; an X x Y tile each."""
    src = src.contiguous()
    pal = _palette(palette, src.device)
    if src.dtype == torch.float32 and src.dim() == 5:
        F, Cn, X, Y, Z = src.shape
        _ck(lib().muvo_panel_voxel_top_logits(_f(src), int(F), int(Cn), int(X), int(Y), int(Z), pal, int(pad), int(padbyte),
                                              *_panel_args(panel, place)))
    elif src.dtype == torch.uint8 and src.dim() == 4:
        F, X, Y, Z = src.shape
        _ck(lib().muvo_panel_voxel_top_grid(_p(src), int(F), int(X), int(Y), int(Z), pal, int(pad), int(padbyte), *_panel_args(panel, place)))
    else:
        raise ValueError(f'panel_voxel_top: logits (F, C, X, Y, Z) float32 or a grid (F, X, Y, Z) uint8, got {tuple(src.shape)} {src.dtype}')


# ---- ray casting through voxel grids (csrc/raycast.hip; include/muvo_hip.h: muvo_raycast, our definition) -------------------------
def raycast_bricks(src):
    """(class grid (F, X, Y, Z) uint8, occupancy bricks (F, words) int64 holding the uint64 words) of src = logits (F, C, X, Y, Z)
    float32 (first maximum over C; the class grid is written by the same kernel) or a class grid (F, X, Y, Z) uint8 (returned as
    it is)."""
    src = src.contiguous()
    L = lib()
    if src.dtype == torch.float32 and src.dim() == 5:
        F, Cn, X, Y, Z = src.shape
        logits = True
    elif src.dtype == torch.uint8 and src.dim() == 4:
        F, X, Y, Z = src.shape
        logits = False
    else:
        raise ValueError(f'raycast_bricks: logits (F, C, X, Y, Z) float32 or a grid (F, X, Y, Z) uint8, got {tuple(src.shape)} {src.dtype}')
    words = int(L.muvo_raycast_brick_words(int(F), int(X), int(Y), int(Z)))
    if words < 0:
        raise ValueError(f'raycast_bricks: {F} frames of {X} x {Y} x {Z} (1..65535 frames, 1..2048 per axis)')
    bricks = torch.empty((F, words // F), dtype=torch.int64, device=src.device)
    if logits:
        grid = torch.empty((F, X, Y, Z), dtype=torch.uint8, device=src.device)
        _ck(L.muvo_raycast_bricks_logits(_f(src), int(F), int(Cn), int(X), int(Y), int(Z), _p(grid), _p(bricks), _i64(words), _st()))
        return grid, bricks
    _ck(L.muvo_raycast_bricks_grid(_p(src), int(F), int(X), int(Y), int(Z), _p(bricks), _i64(words), _st()))
    return src, bricks


def visibility_mark(grid, bricks, rays):
    """The SEEN words (F, words) int64 - layout and bit order of `raycast_bricks` - of the R rays (R, 7) float32 through each of
    the F frames: every cell a ray visits up to and including its first occupied one (include/muvo_hip.h: muvo_visibility_mark,
    our definition).  The entry clears the words itself."""
    F, X, Y, Z = _ray_args(grid, bricks, rays)
    seen = torch.empty_like(bricks)
    _ck(lib().muvo_visibility_mark(_p(grid), _p(bricks), F, X, Y, Z, _f(rays), _i64(rays.shape[0]), _p(seen), _i64(seen.numel()), _st()))
    return seen


def visibility_apply(label, seen, counts=None):
    """The masked label (F, X, Y, Z) uint8 of `label` under the SEEN words of `visibility_mark`: label where it is not 0, 0 where a
    free cell is seen, 255 where it is not.  counts (2,) int64 on the device (free-and-seen, unknown) is added to; None: a fresh
    one.  Returns (masked label, counts)."""
    assert label.dtype == torch.uint8 and label.dim() == 4 and label.is_contiguous()
    F, X, Y, Z = (int(v) for v in label.shape)
    assert seen.dtype == torch.int64 and seen.is_contiguous() and seen.device == label.device
    assert tuple(seen.shape) == (F, ((X + 3) // 4) * ((Y + 3) // 4) * ((Z + 3) // 4)), 'visibility_apply: the words of visibility_mark for this grid'
    if counts is None:
        counts = torch.zeros(2, dtype=torch.int64, device=label.device)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (2,) and counts.is_contiguous() and counts.device == label.device
    out = torch.empty_like(label)
    _ck(lib().muvo_visibility_apply(_p(label), _p(seen), F, X, Y, Z, _p(out), _p(counts), _st()))
    return out, counts


def visible_labels(label, rays, counts=None):
    """bricks + mark + apply for a label grid (F, X, Y, Z) uint8: (masked label, counts)."""
    grid, bricks = raycast_bricks(label)
    return visibility_apply(grid, visibility_mark(grid, bricks, rays), counts)


# ---- voxel labels filled from neighbouring frames (csrc/voxel_aggregate.hip; include/muvo_hip.h: muvo_voxel_aggregate, our definition)
def voxel_cell_map(cfg, factor):
    """The affine map (6,) float64 - scale per axis, then offset per axis - from range-view coordinates (the x, y, z planes of
    range_view_label_1 times LIDAR_RE.SCALE: metres in the ego frame) to the grid coordinates of the voxel labels at scale
    `factor`: g = r / (VOXEL.RESOLUTION factor) + VOXEL.EV_POSITION / factor (include/muvo_hip.h: muvo_voxel_pose_chain)."""
    a = 1.0 / (float(cfg.VOXEL.RESOLUTION) * int(factor))
    return [a, a, a] + [float(v) / int(factor) for v in cfg.VOXEL.EV_POSITION]


def voxel_pose_chain(T, b, s, window, cell_map, fitness=None, status=None, min_fitness=0.0):
    """(mats (b s, 2 window, 12) float64, usable (b s, 2 window) uint8) of the b (s - 1) link matrices T (b (s - 1), 4, 4) float64 on
    the device, p_{t-1} ~ T_t p_t, in the walk order of muvo_voxel_aggregate and in the cell coordinates of `cell_map` (6 numbers:
    voxel_cell_map).  fitness (float64) and status (int64), (b (s - 1),) device tensors as IcpResult holds them, decide with
    min_fitness which links are valid; both None: every finite link is."""
    b, s, window = int(b), int(s), int(window)
    assert T.dtype == torch.float64 and T.is_cuda, 'voxel_pose_chain: float64 link matrices on the device'
    T = T.reshape(-1, 4, 4).contiguous()
    if b < 1 or s < 1 or T.shape[0] != b * (s - 1):
        raise ValueError(f'voxel_pose_chain: {T.shape[0]} link matrices for {b} sequences of {s} frames')
    if (fitness is None) != (status is None):
        raise ValueError('voxel_pose_chain: fitness and status come together or not at all')
    if fitness is not None:
        assert fitness.dtype == torch.float64 and status.dtype == torch.int64 and fitness.device == T.device and status.device == T.device
        assert tuple(fitness.shape) == (T.shape[0],) and tuple(status.shape) == (T.shape[0],), 'voxel_pose_chain: one fitness and one status per link'
        fitness, status = fitness.contiguous(), status.contiguous()
    if window < 1 or window > 64:
        raise ValueError(f'voxel_pose_chain: window {window} outside 1..64')
    cm = [float(v) for v in cell_map]
    if len(cm) != 6:
        raise ValueError('voxel_pose_chain: cell_map is 3 scales and 3 offsets')
    mats = torch.empty((b * s, 2 * window, 12), dtype=torch.float64, device=T.device)
    usable = torch.empty((b * s, 2 * window), dtype=torch.uint8, device=T.device)
    _ck(lib().muvo_voxel_pose_chain(_p(T) if T.numel() else C.c_void_p(0), _p(fitness), _p(status), b, s, C.c_double(float(min_fitness)), window,
                                    (C.c_double * 6)(*cm), _p(mats), _p(usable), _st()))
    return mats, usable


def voxel_aggregate(label, bricks, seen, s, mats, usable, counts=None):
    """The aggregated masked label (F, X, Y, Z) uint8 of `label` (F = b s frames, sequences of s): what visibility_apply writes
    where the frame observed the cell itself; every other cell takes the state of the cell it falls into in the nearest usable
    frame of its sequence that observed it (mats, usable: voxel_pose_chain), 255 if none did.  counts (3,) int64 on the device
    (filled occupied, filled free, still unknown) is added to; None: a fresh one.  Returns (label, counts)."""
    assert label.dtype == torch.uint8 and label.dim() == 4 and label.is_contiguous()
    F, X, Y, Z = (int(v) for v in label.shape)
    words = ((X + 3) // 4) * ((Y + 3) // 4) * ((Z + 3) // 4)
    for t, what in ((bricks, 'raycast_bricks'), (seen, 'visibility_mark')):
        assert t.dtype == torch.int64 and t.is_contiguous() and t.device == label.device
        assert tuple(t.shape) == (F, words), f'voxel_aggregate: the words of {what} for this grid'
    s = int(s)
    if s < 1 or F % s:
        raise ValueError(f'voxel_aggregate: {F} frames are not sequences of {s}')
    assert mats.dtype == torch.float64 and mats.dim() == 3 and mats.shape[0] == F and mats.shape[2] == 12 and mats.shape[1] % 2 == 0 and mats.is_contiguous() \
        and mats.device == label.device, 'voxel_aggregate: mats (F, 2 window, 12) float64 of voxel_pose_chain'
    assert usable.dtype == torch.uint8 and tuple(usable.shape) == tuple(mats.shape[:2]) and usable.is_contiguous() and usable.device == label.device
    if counts is None:
        counts = torch.zeros(3, dtype=torch.int64, device=label.device)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (3,) and counts.is_contiguous() and counts.device == label.device
    out = torch.empty_like(label)
    _ck(lib().muvo_voxel_aggregate(_p(label), _p(bricks), _p(seen), F, s, X, Y, Z, int(mats.shape[1]) // 2, _p(mats), _p(usable), _p(out), _p(counts), _st()))
    return out, counts


def aggregated_labels(label, rays, s, T, window, cell_map, fitness=None, status=None, min_fitness=0.0, counts=None):
    """bricks + mark + chain + aggregate for a label grid (b s, X, Y, Z) uint8: (aggregated masked label, counts)."""
    grid, bricks = raycast_bricks(label)
    seen = visibility_mark(grid, bricks, rays)
    mats, usable = voxel_pose_chain(T, grid.shape[0] // int(s), s, window, cell_map, fitness, status, min_fitness)
    return voxel_aggregate(grid, bricks, seen, s, mats, usable, counts)


def _ray_args(grid, bricks, rays):
    assert grid.dtype == torch.uint8 and grid.dim() == 4 and grid.is_contiguous()
    assert bricks.dtype == torch.int64 and bricks.is_contiguous() and bricks.shape[0] == grid.shape[0]
    assert rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 7 and rays.is_contiguous() and rays.device == grid.device
    return tuple(int(v) for v in grid.shape)


def raycast(grid, bricks, rays):
    """First hits of the R rays (R, 7) float32 in each of the F frames of `raycast_bricks`: (hit (F, R) int32 linear cell index or
    -1, t (F, R) float32, face (F, R) uint8)."""
    F, X, Y, Z = _ray_args(grid, bricks, rays)
    R = rays.shape[0]
    hit = torch.empty((F, R), dtype=torch.int32, device=grid.device)
    t = torch.empty((F, R), dtype=torch.float32, device=grid.device)
    face = torch.empty((F, R), dtype=torch.uint8, device=grid.device)
    _ck(lib().muvo_raycast(_p(grid), _p(bricks), F, X, Y, Z, _f(rays), _i64(R), _p(hit), _f(t), _p(face), _st()))
    return hit, t, face


def panel_voxel_view(grid, bricks, rays, palette, panel, place, pad=0, padbyte=0):
    """Shaded first-hit view of voxel grids through an R x R ray table (R * R, 7): an R x R tile each in a 3-channel panel."""
    F, X, Y, Z = _ray_args(grid, bricks, rays)
    R = math.isqrt(rays.shape[0])
    assert R * R == rays.shape[0], 'panel_voxel_view: a square ray table'
    assert panel.dim() == 4 and panel.shape[1] == 3
    _ck(lib().muvo_panel_voxel_view(_p(grid), _p(bricks), F, X, Y, Z, _f(rays), int(R), _palette(palette, grid.device), int(pad), int(padbyte),
                                    *_panel_args(panel, place)))


def ray_iou_counts(label, label_bricks, pred, pred_bricks, rays, n_classes, resolution, counts, depth, thresholds=(1.0, 2.0, 4.0)):
    """counts (3, C, 3) int64 (threshold x class x tp / fp / fn) and depth (2,) float64 (sum of |dt| in metres, rays) on the
    device are added to, over the R rays through F label and F prediction frames (include/muvo_hip.h: muvo_ray_iou_counts);
    nothing is read back."""
    F, X, Y, Z = _ray_args(label, label_bricks, rays)
    assert _ray_args(pred, pred_bricks, rays) == (F, X, Y, Z), 'ray_iou_counts: label and prediction of one shape'
    Cn = int(n_classes)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (3, Cn, 3) and counts.is_contiguous()
    assert depth.dtype == torch.float64 and tuple(depth.shape) == (2,)
    R = rays.shape[0]
    ws = scratch('ray_iou', max(1, lib().muvo_ray_iou_ws_doubles(_i64(F), _i64(R))), label.device, torch.float64)
    _ck(lib().muvo_ray_iou_counts(_p(label), _p(label_bricks), _p(pred), _p(pred_bricks), F, Cn, X, Y, Z, _f(rays), _i64(R), _fl(resolution),
                                  (C.c_float * 3)(*[float(v) for v in thresholds]), _p(counts), _p(ws), _i64(ws.numel()), _p(depth), _st()))
