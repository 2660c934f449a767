"""Optical flow of the camera frames: the `_flow` block of the reference's `WorldModelTrainer.visualise` (trainer.py:723-752,
1009-1020).  The reference colour-codes cv2.calcOpticalFlowFarneback between consecutive RGB frames of the label, the
reconstruction and every imagined sample, one pair at a time on the host.  Here all pairs of a row segment run as one work list on
the device (ops.optical_flow -> csrc/flow.hip) and the colour coding is fused into the tile writer (ops.flow_colour): only the
finished panel leaves the device.

OUR DEFINITION where the reference delegates to cv2: the flow itself and the colour coding (include/muvo_hip.h: muvo_flow_*;
tests/flow_reference.py restates both).  It is Farneback's method with the reference's parameters, but parity with cv2's
numbers is not pinned.

Panel `_flow`: (b, 3, (1 + rows)(h + 10), (s - 1)(w + 10)) uint8.  Column step - 1 holds the flow label[step - 1] -> label[step]
on top and below it one tile per prediction row i (row 0: the reconstruction, then imagination 0; row i > 0: all-white frames
in the receptive part, then imagination i).  Every tile is the flow of the full h x w frames inside a border of 5 pixels of
byte 204 (the reference crops the 5-pixel pad it added before: `[5:-5]`); there is no separator block.  The reference's
substitution `if i == rf: img1 = rgb_preds_np[0][bs, step - 1]` is restated literally: it compares the ROW index with rf, so
row rf - when there are more than rf imagined samples - takes all its first frames from row 0.  A row without imagined samples
ends after the reconstructed steps; the tiles it does not reach stay 255."""
import json
import os

import torch

PAD, PAD_BYTE = 5, 204
WHITE = -1


def flow_rows(s, rf, n_imagines):
    """The work list of the panel for ONE sample: [row][step - 1] = (first, second) for step = 1 .. L - 1, each a (stack, t) with
    stack 'label' | 'recon' | ('imagine', i) and t the frame's index in that stack, or WHITE.  Row 0 is the label; the length
    L of a prediction row is s with imagined samples and rf without."""
    def frame(i, t):
        if t >= rf:
            return (('imagine', i), t - rf)
        return ('recon', t) if i == 0 else WHITE
    rows = [[(('label', t - 1), ('label', t)) for t in range(1, s)]]
    L = s if n_imagines else rf
    for i in range(max(n_imagines, 1)):
        row = []
        for step in range(1, L):
            first = frame(i, step - 1)
            if i == rf:
                first = frame(0, step - 1)
            row.append((first, frame(i, step)))
        rows.append(row)
    return rows


def _segments(row):
    """runs of consecutive steps of a row whose pairs come from the same two stacks: [(col0, [(first, second), ...])]"""
    def key(pair):
        a, b = (None if f == WHITE else f[0] for f in pair)
        return (a if a is not None else b, b if b is not None else a)
    out = []
    for col, pair in enumerate(row):
        if out and key(out[-1][1][-1]) == key(pair):
            out[-1][1].append(pair)
        else:
            out.append((col, [pair]))
    return out


def panel_jobs(b, s, rf, n_imagines):
    """[(row, col0, stack_a, stack_b, idx_a, idx_b, T)]: one optical_flow call and one tile-writer call each - the T pairs of the
    columns col0 .. col0 + T - 1 of `row` for every sample (sample-major), idx = per-sample frame index or WHITE; a segment of
    two white frames has stacks (None, None): its flow is exactly zero, an all-255 tile."""
    jobs = []
    for r, row in enumerate(flow_rows(s, rf, n_imagines)):
        for col0, pairs in _segments(row):
            sa = next((p[0][0] for p in pairs if p[0] != WHITE), None)
            sb = next((p[1][0] for p in pairs if p[1] != WHITE), None)
            ia = [WHITE if p[0] == WHITE else p[0][1] for p in pairs]
            ib = [WHITE if p[1] == WHITE else p[1][1] for p in pairs]
            jobs.append((r, col0, sa, sb, ia, ib, len(pairs)))
    return jobs


def assemble(b, s, rf, n_imagines, h, w, tiles_fn):
    """The panel on the host from tiles_fn(stack_a, stack_b, pairs) -> (len(pairs), 3, h + 10, w + 10) uint8 numpy, pairs =
    [(sample, idx_a, idx_b)]: the layout the device path follows, for tests and as documentation."""
    import numpy as np
    th, tw = h + 2 * PAD, w + 2 * PAD
    out = np.full((b, 3, (1 + max(n_imagines, 1)) * th, (s - 1) * tw), 255, np.uint8)
    for r, col0, sa, sb, ia, ib, T in panel_jobs(b, s, rf, n_imagines):
        pairs = [(n, ia[k], ib[k]) for n in range(b) for k in range(T)]
        tiles = tiles_fn(sa, sb, pairs)
        for q, (n, _, _) in enumerate(pairs):
            c = col0 + q % T
            out[n, :, r * th:(r + 1) * th, c * tw:(c + 1) * tw] = tiles[q]
    return out


def _stacks(batch, output, output_imagines):
    label = batch['rgb_label_1'].float()
    recon = output['rgb_1'].detach().float()
    imagines = [im['rgb_1'].detach().float() for im in (output_imagines or [])]
    b, s, c, h, w = label.shape
    rf = recon.shape[1]
    for x in [recon] + imagines:
        if x.shape[0] != b or x.shape[2:] != label.shape[2:]:
            raise ValueError(f'flow: a prediction of shape {tuple(x.shape)} for a label of {tuple(label.shape)}')
    if c != 3:
        raise ValueError(f'flow: RGB frames, got {c} channels')
    if imagines and any(rf + im.shape[1] != s for im in imagines):
        raise ValueError(f'flow: {rf} reconstructed + {imagines[0].shape[1]} imagined frames for a label of {s}')
    if not imagines and rf > s:
        raise ValueError(f'flow: {rf} reconstructed frames for a label of {s}')
    stacks = {'label': label, 'recon': recon}
    for i, im in enumerate(imagines):
        stacks[('imagine', i)] = im
    return {k: v.reshape(v.shape[0] * v.shape[1], 3, h, w) for k, v in stacks.items()}, {k: v.shape[1] for k, v in stacks.items()}, (b, s, rf, len(imagines), h, w)


def _indices(b, length, idx):
    """per-sample frame indices -> indices into the (b * length) stack, sample-major"""
    return [WHITE if t == WHITE else n * length + t for n in range(b) for t in idx]


def flow_panel(batch, output, output_imagines):
    """the `_flow` panel of one batch as a (b, 3, (1 + rows)(h + 10), (s - 1)(w + 10)) uint8 device tensor"""
    from muvo_amd import ops
    frames, lengths, (b, s, rf, n_im, h, w) = _stacks(batch, output, output_imagines)
    th, tw = h + 2 * PAD, w + 2 * PAD
    panel = torch.full((b, 3, (1 + max(n_im, 1)) * th, max(s - 1, 0) * tw), 255, dtype=torch.uint8, device=frames['label'].device)
    for r, col0, sa, sb, ia, ib, T in panel_jobs(b, s, rf, n_im):
        place = ops.tile_place(panel, T, col0, y0=r * th, xstep=tw)
        if sa is None and sb is None:                         # two white frames: zero flow
            ops.panel_fill(b * T, h, w, 255, panel, place, PAD, PAD_BYTE)
            continue
        sa, sb = (sa if sa is not None else sb), (sb if sb is not None else sa)
        flow = ops.optical_flow(frames[sa], frames[sb], _indices(b, lengths[sa], ia), _indices(b, lengths[sb], ib))
        ops.flow_colour(flow, panel, place, PAD, PAD_BYTE)
    return panel


class FlowMetric:
    """`predict --mode test --optical-flow`: per loader the mean endpoint error in pixels between the flow of the recorded
    frames and the flow of the predicted frames over the same step - `flow_epe` over the reconstructed steps 1 .. rf - 1,
    `flow_epe_imagine` over the steps rf + 1 .. s - 1 of the first imagined sample - without the five border rows and columns,
    and next to each the mean magnitude of the recorded flow, so the figure can be read as a ratio.  `update` is the per-batch
    hook of predict.run and only queues kernels (fp64 sums stay on the device); `result()` reads them once per loader."""
    KEYS = ('flow_epe', 'flow_epe_imagine', 'flow_magnitude', 'flow_magnitude_imagine', 'pairs', 'pairs_imagine')

    def __init__(self, cfg=None, prefix='test'):
        self.cfg, self.prefix = cfg, prefix
        self.loader = None
        self.acc = {}

    def start_loader(self, idx):
        self.loader = str(idx)
        self.acc[self.loader] = dict(sums=None, pairs=[0, 0])

    def _add(self, a, which, frames, lengths, b, key, steps):
        from muvo_amd import ops
        if not steps:
            return
        stack, offset = key
        rec = ops.optical_flow(frames['label'], frames['label'], _indices(b, lengths['label'], [t - 1 for t in steps]),
                               _indices(b, lengths['label'], steps))
        idx = [t - offset for t in steps]
        pred = ops.optical_flow(frames[stack], frames[stack], _indices(b, lengths[stack], [t - 1 for t in idx]), _indices(b, lengths[stack], idx))
        ops.flow_epe(rec, pred, a['sums'][which])
        a['pairs'][which] += b * len(steps)

    def update(self, i, batch, output, output_imagines):
        if self.loader is None:
            self.start_loader(0)
        frames, lengths, (b, s, rf, n_im, h, w) = _stacks(batch, output, output_imagines[:1] if output_imagines else [])
        a = self.acc[self.loader]
        if a['sums'] is None:
            a['sums'] = torch.zeros(2, 3, dtype=torch.float64, device=frames['label'].device)
        with torch.no_grad():
            self._add(a, 0, frames, lengths, b, ('recon', 0), list(range(1, rf)))
            if n_im:
                self._add(a, 1, frames, lengths, b, (('imagine', 0), rf), list(range(rf + 1, s)))

    def result(self):
        out = {}
        for idx, a in self.acc.items():
            sums = a['sums'].cpu().tolist() if a['sums'] is not None else [[0.0, 0.0, 0.0]] * 2
            (e0, m0, n0), (e1, m1, n1) = sums
            out[f'{self.prefix}{idx}_flow_epe'] = e0 / n0 if n0 else 0.0
            out[f'{self.prefix}{idx}_flow_epe_imagine'] = e1 / n1 if n1 else 0.0
            out[f'{self.prefix}{idx}_flow_magnitude'] = m0 / n0 if n0 else 0.0
            out[f'{self.prefix}{idx}_flow_magnitude_imagine'] = m1 / n1 if n1 else 0.0
            out[f'{self.prefix}{idx}_flow_pairs'] = a['pairs'][0]
            out[f'{self.prefix}{idx}_flow_pairs_imagine'] = a['pairs'][1]
        return out

    def write(self, out_dir):
        path = os.path.join(out_dir, 'optical_flow.json')
        with open(path, 'w') as fh:
            json.dump(self.result(), fh, indent=1, sort_keys=True)
            fh.write('\n')
        return path
