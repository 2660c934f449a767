"""Fixture generator for the prediction panels (runs only where the reference is available): imports the real reference
through the import stubs of oracle/refimport, calls its `WorldModelTrainer.visualise` and `pcd_xy_image` unbound on a
namespace with a recording writer, and stores the bytes TensorBoard's writer would make of what it was handed in
tests/golden/visualise_ref.npz.  The inputs are the seeded ones of tests/visualise_reference.fixture_inputs; the heads that need
cv2, open3d or matplotlib (RGB, lidar reconstruction, voxels) are off.

Usage: python tools/make_golden_visualise.py"""
import os
import sys
from types import SimpleNamespace

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

from oracle.refimport.make_golden import import_reference  # noqa: E402
import visualise_reference as VR  # noqa: E402


class Recorder:
    def __init__(self):
        self.seen = {}

    def add_images(self, name, tensor, global_step=None):
        self.seen[name] = VR.to_u8(tensor.detach().cpu().numpy())

    def add_video(self, name, tensor, global_step=None, fps=None):
        self.seen[name] = VR.to_u8(tensor.detach().cpu().numpy())


def main():
    ref_trainer, ref_config = import_reference()
    cfg = ref_config._C.clone()
    cfg.SEMANTIC_SEG.ENABLED = cfg.LIDAR_SEG.ENABLED = cfg.SEMANTIC_IMAGE.ENABLED = cfg.DEPTH.ENABLED = cfg.MODEL.ROUTE.ENABLED = True
    cfg.EVAL.RGB_SUPERVISION = cfg.LIDAR_RE.ENABLED = cfg.VOXEL_SEG.ENABLED = False
    out = {}
    for n in (0, 1, 2):
        batch, output, imagines = VR.fixture_inputs(n)
        rec = Recorder()
        this = SimpleNamespace(cfg=cfg, global_step=0, rf=VR.FIXTURE['rf'])
        ref_trainer.WorldModelTrainer.visualise(this, batch, output, imagines, 0, prefix='train', writer=rec)
        assert sorted(rec.seen) == sorted(f'train_outputs{k}' for k in VR.FIXTURE_SUFFIXES), sorted(rec.seen)
        for k in VR.FIXTURE_SUFFIXES:
            out[f'n{n}{k}'] = rec.seen[f'train_outputs{k}']
            print(f'n{n}{k}', out[f'n{n}{k}'].shape)
    this = SimpleNamespace(cfg=SimpleNamespace(LIDAR_RE=SimpleNamespace(SCALE=VR.SCALE)))
    image, _, _ = ref_trainer.WorldModelTrainer.pcd_xy_image(this, VR.fixture_range_view())
    out['pcd_xy_image'] = VR.to_u8(image.numpy())
    path = os.path.join(REPO, 'tests', 'golden', 'visualise_ref.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
