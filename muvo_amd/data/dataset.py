"""Dataset reader for recorded CARLA runs: counterpart of the reference's muvo/data/dataset.py (`DataModule`, `CarlaDataset`,
lines 19-369), split where the reference is not:

  host    `CarlaDataset.read_raw(i)`: file I/O and decoding only (PIL for the PNGs, np.load for the point and voxel files, the
          action -> throttle_brake rule, reward clipping) -> raw arrays of one sequence;
  device  `input_pipeline.prepare_frames`: a whole batch of raw frames -> the reference's batch dict (bird's-eye-view planes,
          labels and instance components, range view, dense voxel grid, depth / semantic image) in a handful of launches.

`BatchLoader` joins the two: a pool of at most min(N_WORKERS, 16) host threads (no worker processes: only the training process
opens the GPU) reads raw frames, two batches ahead, into pinned staging buffers; the copy and the preparation of batch k+1 are queued
before batch k is handed out - on the consumer's stream by default, with input_stream=True on an input stream of the loader's
own with a stream event for the handover (the measurement behind the default).  `points_raw` / `num_points`
(MODEL.LIDAR.POINT_PILLAR) are not built: that configuration is outside the built rows (models/mile.py raises).
pandas and PIL are imported where a recording is opened, not at module import."""
import contextlib
import os
import random
from concurrent.futures import ThreadPoolExecutor
from glob import glob

import numpy as np
import torch

CARLA_FPS = 10                                  # constants.py:3
MAX_HOST_THREADS = 16


def calculate_geometry_from_config(cfg):
    """dataset.py:372-385 + geometry_utils.py:64-91: float32 intrinsics (3, 3) and extrinsics (4, 4) of the one camera."""
    fov = cfg.IMAGE.FOV
    h, w = cfg.IMAGE.SIZE
    forward, right, up = cfg.IMAGE.CAMERA_POSITION
    pitch, yaw, roll = cfg.IMAGE.CAMERA_ROTATION
    assert pitch == yaw == roll == 0.0
    f = w / (2 * np.tan(fov * np.pi / 360.0))
    intrinsics = np.float32([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]])
    extrinsics = np.float32([[0, 0, 1, forward], [-1, 0, 0, -right], [0, -1, 0, up], [0, 0, 0, 1]])
    return intrinsics, extrinsics


def _png(Image, path):
    with Image.open(path) as im:
        return np.asarray(im)


class FrameError(RuntimeError):
    """A frame file is missing or cannot be decoded (the reference prints a line and silently shortens the sequence)."""


class CarlaDataset:
    """Sequences of `sequence_length` frames, `STRIDE_SEC` apart, from every run below `<root>/<DATASET.VERSION>/<mode>` that has a
    `pd_dataframe.pkl` and passes the reward filter.  Same arguments, `data`, `data_pointers` and `len()` as the reference's class."""

    def __init__(self, cfg, mode='train', sequence_length=1, dataset_root=None, towns_filter='*', runs_filter='*'):
        import pandas as pd
        if cfg.MODEL.LIDAR.POINT_PILLAR.ENABLED:
            raise NotImplementedError('MODEL.LIDAR.POINT_PILLAR: points_raw / num_points are not built')
        self.cfg, self.mode, self.sequence_length = cfg, mode, sequence_length
        self.dataset_path = os.path.join(dataset_root, cfg.DATASET.VERSION, mode)
        self.intrinsics, self.extrinsics = calculate_geometry_from_config(cfg)
        # run id 'town/run' -> data frame, in sorted order of towns, then runs (the order fixes the order of the pointers)
        tables = sorted(glob(os.path.join(self.dataset_path, towns_filter, runs_filter, 'pd_dataframe.pkl')),
                        key=lambda f: f.split(os.sep)[-3:-1])
        self.data = {'/'.join(f.split(os.sep)[-3:-1]): pd.read_pickle(f) for f in tables}
        self.n_filtered_run = 0
        self.data_pointers = self.get_data_pointers()

    def get_data_pointers(self):
        """[(run id, [frame indices])]: every start frame from FILTER_BEGINNING_OF_RUN_SEC on whose whole sequence fits into the
        run, for the runs whose mean reward reaches FILTER_NORM_REWARD; thinned by EVAL.DATASET_REDUCTION with the reference's
        draw (random.seed(0), random.sample)."""
        step = int(self.cfg.DATASET.STRIDE_SEC * CARLA_FPS)
        first = int(CARLA_FPS * self.cfg.DATASET.FILTER_BEGINNING_OF_RUN_SEC)
        span = step * self.sequence_length
        pointers, rejected = [], 0
        for run_id, table in self.data.items():
            rewards = table['reward']
            if rewards.sum() / len(rewards) < self.cfg.DATASET.FILTER_NORM_REWARD:
                rejected += 1
                continue
            pointers += [(run_id, list(range(start, start + span, step))) for start in range(first, len(table) - span)]
        self.n_filtered_run = rejected
        print(f'{self.dataset_path}: {len(self.data)} runs, {rejected} below the reward filter, {len(pointers)} sequences')
        if self.cfg.EVAL.DATASET_REDUCTION:
            random.seed(0)
            pointers = random.sample(pointers, int(len(pointers) / self.cfg.EVAL.DATASET_REDUCTION_FACTOR))
        return pointers

    def __len__(self):
        return len(self.data_pointers)

    # ---- host side: files -> raw arrays ------------------------------------------------------------------------------------
    def needs_depth_semantic(self):
        return bool(self.cfg.LOSSES.RGB_INSTANCE or self.cfg.SEMANTIC_IMAGE.ENABLED or self.cfg.DEPTH.ENABLED)

    def read_frame(self, run_id, t):
        """The raw arrays of one frame; nothing is computed beyond decoding, the throttle_brake rule and the reward clip."""
        from PIL import Image
        row = self.data[run_id].iloc[t]
        base = os.path.join(self.dataset_path, run_id)
        what = 'data frame row'
        try:
            out = {'n_classes': int(row['n_classes'])}
            what = row['image_path']
            out['image'] = _png(Image, os.path.join(base, what))                      # (H, W, 3) uint8
            what = row['routemap_path']
            out['route_map'] = _png(Image, os.path.join(base, what))                  # (h, w) uint8
            what = row['birdview_path']
            out['birdview_int'] = _png(Image, os.path.join(base, what)).astype(np.int32)
            what = row['points_semantic_path']
            pcd = np.load(os.path.join(base, what), allow_pickle=True).item()
            out['points_xyz'] = np.ascontiguousarray(pcd['points_xyz'], dtype=np.float32)
            out['obj_tag'] = np.ascontiguousarray(pcd['ObjTag'], dtype=np.uint8)
            if len(out['points_xyz']) != len(out['obj_tag']) or out['points_xyz'].shape[1:] != (3,):
                raise ValueError('points_xyz / ObjTag shapes do not match')
            if self.cfg.VOXEL_SEG.ENABLED:
                what = row['voxel_path']
                vox = np.load(os.path.join(base, what))
                if vox.ndim != 2 or vox.shape[1] != 4:
                    raise ValueError(f'voxel rows must be (Q, 4), got {vox.shape}')
                out['voxel_rows'] = vox.astype(np.int64)
            if self.needs_depth_semantic():
                what = row['depth_semantic_path']
                out['depth_semantic'] = _png(Image, os.path.join(base, what))         # (H, W, 4) uint8
                if out['depth_semantic'].ndim != 3 or out['depth_semantic'].shape[2] != 4:
                    raise ValueError('depth_semantic must be an RGBA image')
            what = 'data frame row'
            gas, steer, brake = row['action']
            out['steering'] = np.float32([steer])
            out['throttle_brake'] = np.float32([gas if gas > 0 else -brake])       # braking shows as negative throttle
            out['speed'] = np.asarray(row['speed'])
            out['reward'] = np.clip(np.float32([row['reward']]), -1.0, 1.0)
            out['value_function'] = np.float32([row['value']])
        except Exception as e:
            raise FrameError(f'{self.dataset_path}: run {run_id}, frame {t}: cannot read {what}: {type(e).__name__}: {e}') from e
        return out

    def read_raw(self, i):
        """Raw arrays of sequence i, stacked over its frames: `image` (s, 3, H, W) and `route_map` (s, 3, h, w) uint8 in the
        batch's layout (the transposition / grey-to-RGB broadcast is part of the one copy into the stack), `birdview_int`
        (s, H, W) int32 + `n_classes`, `points_xyz` (s, Pmax, 3) float32 / `obj_tag` (s, Pmax) uint8 zero-padded with
        `num_points` (s,) int32, `voxel_rows` (s, Qmax, 4) int64 with `num_voxels`, `depth_semantic` (s, H, W, 4) uint8 when a
        head needs it, the per-frame scalars (s, 1) and the camera geometry."""
        run_id, indices = self.data_pointers[i]
        return stack_frames([self.read_frame(run_id, t) for t in indices], self.intrinsics, self.extrinsics)

    def __getitem__(self, i):
        """What the reference's __getitem__ returns: CPU tensors (s, ...) of every batch key.  The preparation runs on the
        GPU (there is no host implementation); training takes batches from `BatchLoader` instead."""
        from .. import input_pipeline as IP
        dev = torch.device('cuda', torch.cuda.current_device())
        raw = collate_raw([self.read_raw(i)])
        batch = IP.prepare_frames({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in raw.items()}, self.cfg)
        return {k: v[0].cpu() for k, v in batch.items()}


def _pad_stack(arrays, dtype):
    n = max(len(a) for a in arrays)
    out = np.zeros((len(arrays), n) + arrays[0].shape[1:], dtype=dtype)
    for f, a in enumerate(arrays):
        out[f, :len(a)] = a
    return out, np.array([len(a) for a in arrays], dtype=np.int32)


def stack_frames(frames, intrinsics, extrinsics):
    s = len(frames)
    n_classes = frames[0]['n_classes']
    assert all(f['n_classes'] == n_classes for f in frames), 'n_classes differs inside a sequence'
    out = {'n_classes': n_classes}
    out['image'] = np.stack([f['image'].transpose(2, 0, 1) for f in frames])
    out['route_map'] = np.stack([np.broadcast_to(f['route_map'][None], (3,) + f['route_map'].shape) for f in frames])
    out['birdview_int'] = np.stack([f['birdview_int'] for f in frames])
    out['points_xyz'], out['num_points'] = _pad_stack([f['points_xyz'] for f in frames], np.float32)
    out['obj_tag'], _ = _pad_stack([f['obj_tag'] for f in frames], np.uint8)
    if 'voxel_rows' in frames[0]:
        out['voxel_rows'], out['num_voxels'] = _pad_stack([f['voxel_rows'] for f in frames], np.int64)
    if 'depth_semantic' in frames[0]:
        out['depth_semantic'] = np.stack([f['depth_semantic'] for f in frames])
    for k in ('steering', 'throttle_brake', 'speed', 'reward', 'value_function'):
        out[k] = np.stack([f[k] for f in frames])
    out['intrinsics'] = np.broadcast_to(intrinsics, (s,) + intrinsics.shape).copy()
    out['extrinsics'] = np.broadcast_to(extrinsics, (s,) + extrinsics.shape).copy()
    return out


PADDED = {'points_xyz': 'num_points', 'obj_tag': 'num_points', 'voxel_rows': 'num_voxels'}


def collate_raw(raws, buffers=None):
    """b raw sequences -> one dict of (b, s, ...) CPU tensors; the padded arrays are padded to the batch's longest frame.
    buffers: `PinnedBuffers` to stage into (page-locked memory the copy engine reads directly); None: ordinary tensors."""
    b = len(raws)
    assert all(r['n_classes'] == raws[0]['n_classes'] for r in raws), 'n_classes differs inside a batch'
    out = {'n_classes': raws[0]['n_classes']}
    for k, first in raws[0].items():
        if k == 'n_classes':
            continue
        shape = list(first.shape)
        if k in PADDED:
            shape[1] = max(r[k].shape[1] for r in raws)
        dst = buffers.get(k, (b, *shape), first.dtype) if buffers is not None else torch.zeros((b, *shape), dtype=torch.from_numpy(first[:0]).dtype)
        view = dst.numpy()
        for j, r in enumerate(raws):
            if k in PADDED:
                n = r[k].shape[1]
                view[j, :, :n] = r[k]
                view[j, :, n:] = 0
            else:
                view[j] = r[k]
        out[k] = dst
    return out


class PinnedBuffers:
    """Page-locked staging memory of one batch slot, grown on demand and reused."""

    def __init__(self):
        self.store = {}
        self.event = None           # recorded after the last upload from this slot; waited for before the slot is rewritten

    def get(self, name, shape, np_dtype):
        dtype = torch.from_numpy(np.empty(0, dtype=np_dtype)).dtype
        n = int(np.prod(shape))
        cur = self.store.get(name)
        if cur is None or cur.numel() < n or cur.dtype != dtype:
            cur = self.store[name] = torch.empty(max(n, 1), dtype=dtype, pin_memory=True)
        return cur[:n].view(*shape)


class BatchLoader:
    """Iterator of device batches over `dataset`.  sampler: the indices to visit in order (validation / test ranges); None:
    a permutation seeded by (seed, epoch).  The order is sharded rank::world_size, cut into batches of batch_size, and the last
    partial batch is dropped.  input_stream=True queues the copies and the preparation on a stream of the loader's own instead of
    the consumer's."""
    SLOTS = 3

    def __init__(self, dataset, batch_size, device, sampler=None, seed=0, rank=0, world_size=1, n_workers=4, input_stream=False):
        self.dataset, self.batch_size, self.device = dataset, int(batch_size), torch.device(device)
        self.sampler, self.seed, self.rank, self.world_size = sampler, seed, rank, world_size
        self.n_threads = max(1, min(int(n_workers), MAX_HOST_THREADS))
        self.use_input_stream = input_stream
        self.epoch = 0
        self._stream = None
        self._slots = None

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def order(self, epoch=None):
        n = len(self.dataset)
        if self.sampler is not None:
            idx = [int(i) for i in self.sampler]
        else:
            idx = np.random.RandomState((self.seed + 1000003 * (self.epoch if epoch is None else epoch)) % (2 ** 32)).permutation(n).tolist()
        return idx[self.rank::self.world_size]

    def batch_indices(self, epoch=None):
        idx = self.order(epoch)
        nb = len(idx) // self.batch_size
        return [idx[k * self.batch_size:(k + 1) * self.batch_size] for k in range(nb)]

    def __len__(self):
        return len(self.order()) // self.batch_size

    def input_stream(self):
        """Created on first use, and only when a loader runs (the creation order of side streams matters)."""
        if self._stream is None and self.use_input_stream:
            self._stream = torch.cuda.Stream(device=self.device)
        return self._stream

    def upload(self, host):
        """Queues copy + preparation of one staged batch; returns (batch dict on the device, event recorded behind it)."""
        from .. import input_pipeline as IP
        st = self.input_stream()
        with (torch.cuda.stream(st) if st is not None else contextlib.nullcontext()):
            raw = {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in host.items()}
            batch = IP.prepare_frames(raw, self.dataset.cfg)
            ev = torch.cuda.Event()
            ev.record()
        return batch, ev

    def __iter__(self):
        return self.iterate()

    def iterate(self, skip=0):
        """The batches of the current epoch from number `skip` on."""
        batches = self.batch_indices()[skip:]
        if not batches:
            return
        pinned = self.device.type == 'cuda'
        if self._slots is None:
            self._slots = [PinnedBuffers() if pinned else None for _ in range(self.SLOTS)]
        slots = self._slots

        ds = self.dataset

        def stage(reads, slot):
            raws = [stack_frames([r.result() for r in seq], ds.intrinsics, ds.extrinsics) for seq in reads]
            if slot is not None and slot.event is not None:
                slot.event.synchronize()          # the copy engine has finished with this slot's previous content
            return collate_raw(raws, slot)

        with ThreadPoolExecutor(max_workers=self.n_threads) as pool:
            queued = {}

            def submit(k):
                # one task per frame file set, queued before the `stage` task that waits for them (so it cannot starve them)
                reads = [[pool.submit(ds.read_frame, ds.data_pointers[i][0], t) for t in ds.data_pointers[i][1]] for i in batches[k]]
                queued[k] = reads
                return pool.submit(stage, reads, slots[k % self.SLOTS])

            staged = {k: submit(k) for k in range(min(2, len(batches)))}
            try:
                ready = self._upload_slot(staged.pop(0).result(), slots[0])
                queued.pop(0)
                for k in range(len(batches)):
                    cur, ev = ready
                    if k + 2 < len(batches):
                        staged[k + 2] = submit(k + 2)
                    if k + 1 < len(batches):      # queued before step k is: copy and preparation overlap it
                        ready = self._upload_slot(staged.pop(k + 1).result(), slots[(k + 1) % self.SLOTS])
                        queued.pop(k + 1)
                    if self._stream is not None:
                        main = torch.cuda.current_stream(self.device)
                        main.wait_event(ev)
                        for v in cur.values():
                            v.record_stream(main)
                    yield cur
            finally:
                # a consumer that stops early (validation takes the first batches of a loader): what is still queued is dropped -
                # the staging tasks and the file reads behind them - so the pool's threads end with the reads that are running
                for f in staged.values():
                    f.cancel()
                for reads in queued.values():
                    for seq in reads:
                        for r in seq:
                            r.cancel()

    def _upload_slot(self, host, slot):
        batch, ev = self.upload(host)
        if slot is not None:
            slot.event = ev
        return batch, ev


class DataModule:
    """The five datasets and three loader groups of the reference's DataModule (dataset.py:19-141) without Lightning; the loaders
    yield device batches.  Attribute names (`train_dataset`, `val_dataset_0..2`, `test_dataset`, `*_sampler*`) are the reference's."""
    # split -> (attribute, sampler (start, step)); the test set is the training split again.  dataset.py:60-68
    VAL = (('val0', 0, 50), ('val1', 1500, 50), ('val2', 3000, 50))
    TEST = ((0, 900), (1500, 600), (0, 150))

    def __init__(self, cfg, dataset_root=None, device=None, rank=0, world_size=1, seed=0, input_stream=False):
        self.cfg = cfg
        self.batch_size = cfg.BATCHSIZE
        self.sequence_length = cfg.RECEPTIVE_FIELD + cfg.FUTURE_HORIZON
        self.dataset_root = dataset_root or cfg.DATASET.DATAROOT
        self.device = device if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.rank, self.world_size, self.seed, self.input_stream = rank, world_size, seed, input_stream
        self.train_dataset = self.test_dataset = None
        self.train_sampler = None                     # None: shuffled
        for n in range(3):
            setattr(self, f'val_dataset_{n}', None)

    def setup(self, stage=None):
        def open_split(mode):
            return CarlaDataset(self.cfg, mode=mode, sequence_length=self.sequence_length, dataset_root=self.dataset_root)
        self.train_dataset = open_split('train')
        for n, (mode, start, step) in enumerate(self.VAL):
            ds = open_split(mode)
            setattr(self, f'val_dataset_{n}', ds)
            setattr(self, f'val_sampler_{n}', range(start, len(ds), step))
        self.test_dataset = open_split('train')
        for n, (start, step) in enumerate(self.TEST):
            setattr(self, f'test_sampler_{n}', range(start, len(self.test_dataset), step))

    def _loader(self, dataset, sampler, sharded=False):
        return BatchLoader(dataset, self.batch_size, self.device, sampler=sampler, seed=self.seed, rank=self.rank if sharded else 0,
                           world_size=self.world_size if sharded else 1, n_workers=self.cfg.N_WORKERS, input_stream=self.input_stream)

    def train_dataloader(self):
        return self._loader(self.train_dataset, self.train_sampler, sharded=True)

    def val_dataloader(self):
        return [self._loader(d, s) for d, s in ((self.val_dataset_0, self.val_sampler_0), (self.val_dataset_1, self.val_sampler_1),
                                                (self.val_dataset_2, self.val_sampler_2))]

    def test_dataloader(self):
        return [self._loader(self.test_dataset, s) for s in (self.test_sampler_0, self.test_sampler_1, self.test_sampler_2)]

    def train_batches(self, start=0):
        """Endless stream of training batches: epoch after epoch, each with its own permutation.  start: number of batches already
        consumed (a resumed run continues the order where the interrupted one stopped)."""
        loader = self.train_dataloader()
        per_epoch = len(loader)
        if per_epoch == 0:
            raise RuntimeError(f'{self.train_dataset.dataset_path}: {len(self.train_dataset)} sequences are fewer than one batch '
                               f'of {self.batch_size} per rank')
        epoch, skip = divmod(int(start), per_epoch)
        while True:
            loader.set_epoch(epoch)
            yield from loader.iterate(skip)
            epoch, skip = epoch + 1, 0
