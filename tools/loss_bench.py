"""The loss block of forward_train alone, torch expressions against the fused kernels (csrc/losses.hip):
forward + backward in ms (device events, 5 warm-up runs, median of 20), then one whole forward_train +
backward step (S3DIS model section, full model, fp32) with SoftGroup.use_fused_losses off and on, interleaved.
Writes profiles/loss_bench.txt.
Usage (GPU box): python tools/loss_bench.py [--out profiles/loss_bench.txt] [--points 100000]"""
import argparse
import copy
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from softgroup_amd import ops, synthetic  # noqa: E402
from softgroup_amd.model import SoftGroup  # noqa: E402
from softgroup_amd.model.softgroup import _assign_proposals  # noqa: E402
from softgroup_amd.ops import losses as fused  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s, MI355X specification
DEV = 'cuda'


def timed(fn, warmup=5, runs=20):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def point_wise(n, c, lines):
    torch.manual_seed(n + c)
    s = torch.randn(n, c, device=DEV, requires_grad=True)
    o = torch.randn(n, 3, device=DEV, requires_grad=True)
    ol = torch.randn(n, 3, device=DEV)
    y = torch.randint(0, c, (n, ), device=DEV)
    y[::7] = -100
    inst = torch.randint(0, 50, (n, ), device=DEV)
    inst[::3] = -100
    w = torch.rand(c, device=DEV) + 0.1

    def step(f):
        def run():
            s.grad = o.grad = None
            sem, off = f(s, o, y, inst, ol, w, -100)
            (sem + off).backward()
        return run

    t_torch = timed(step(fused._point_wise_loss_torch))
    t_fused = timed(step(ops.point_wise_loss))
    # traffic floor of the two fused kernels: the forward reads n (c + 6) 4 + 16 n bytes, the backward reads the
    # same and writes n (c + 3) 4
    floor = 2 * (n * (c + 6) * 4 + 16 * n) + n * (c + 3) * 4
    lines.append(f'point-wise  N={n:7d} C={c:2d}   torch {t_torch:7.3f} ms   fused {t_fused:7.3f} ms   '
                 f'x{t_torch / t_fused:5.2f}   fused moves >= {floor / 1e6:6.1f} MB: {floor / (t_fused * 1e-3) / 1e9:7.1f} GB/s '
                 f'= {100 * floor / (t_fused * 1e-3) / HBM_PEAK:4.1f} % of the HBM peak (events around forward + '
                 f'backward, launch gaps and autograd included)')


def instance(m, p, g, k1, lines):
    torch.manual_seed(m)
    cls_scores = torch.randn(p, k1, device=DEV, requires_grad=True)
    iou_scores = torch.randn(p, k1, device=DEV, requires_grad=True)
    mask_scores = (3 * torch.randn(m, k1, device=DEV)).requires_grad_(True)
    ious_cluster = torch.rand(p, g, device=DEV)
    ious_pred = torch.rand(p, g, device=DEV)
    instance_cls = torch.randint(0, k1 - 1, (g, ), device=DEV)
    instance_cls[::5] = -100
    bidx = torch.randint(0, p, (m, ), device=DEV, dtype=torch.int32).sort()[0]
    mask_label = torch.randint(-1, 2, (m, ), device=DEV).float()

    def step(assign, loss_fn):
        def run():
            cls_scores.grad = iou_scores.grad = mask_scores.grad = None
            labels = assign()
            out = loss_fn(cls_scores, mask_scores, iou_scores, labels, bidx, mask_label, instance_cls,
                          lambda sig: ious_pred, -100, k1 - 1)
            (out['cls_loss'] + out['mask_loss'] + out['iou_score_loss']).backward()
        return run

    t_torch = timed(step(lambda: _assign_proposals(ious_cluster, instance_cls, instance_cls != -100, 0.5, True, 0.0, k1 - 1),
                         fused._instance_losses_torch))
    t_fused = timed(step(lambda: ops.assign_proposals(ious_cluster, instance_cls, -100, 0.5, True, 0.0, k1 - 1),
                         ops.instance_losses))
    lines.append(f'instance    M={m:7d} P={p} G={g} K+1={k1}   torch {t_torch:7.3f} ms   fused {t_fused:7.3f} ms   '
                 f'x{t_torch / t_fused:5.2f}   (assignment + cls / mask / iou_score losses, mask-IoU kernels excluded)')


def whole_step(points, lines):
    cfg = copy.deepcopy(synthetic.S3DIS_MODEL_CFG)
    cfg['test_cfg']['x4_split'] = False
    cfg['fixed_modules'] = []
    xyz, rgb, inst = synthetic.scene_s2(seed=21, n=points)
    batch = synthetic.make_batch(xyz, rgb, instance_labels=inst)
    batch['semantic_labels'] = batch['semantic_labels'].clamp(max=12)
    batch['instance_cls'] = batch['instance_cls'].clamp(max=12)
    torch.manual_seed(0)
    model = SoftGroup(**cfg).cuda()
    with torch.no_grad():
        model.semantic_linear[-1].weight.normal_(0, 20.0)
    model.train()
    last = {}

    def step(on):
        def run():
            SoftGroup.use_fused_losses = on
            model.zero_grad(set_to_none=True)
            torch.manual_seed(1)
            loss, log = model(batch, return_loss=True)
            loss.backward()
            last[on] = log
        return run

    default = SoftGroup.use_fused_losses
    try:
        times = {False: [], True: []}
        for _ in range(3):                       # interleaved: both legs see the same machine
            for on in (False, True):
                times[on].append(timed(step(on), warmup=3, runs=10))
    finally:
        SoftGroup.use_fused_losses = default
    for on in (False, True):
        lines.append(f'forward_train + backward, {points} points, full model fp32, fused losses {"on " if on else "off"}: '
                     f'median {statistics.median(times[on]):7.2f} ms   (three blocks of 10: '
                     + ' '.join(f'{t:.2f}' for t in times[on]) + f')   loss {last[on]["loss"]:.6f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loss_bench.txt'))
    ap.add_argument('--points', type=int, default=100000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('loss_bench needs the GPU: nothing is measured without one')
    lines = [f'tools/loss_bench.py on {torch.cuda.get_device_name(0)}: forward + backward, median of 20 (ms)']
    point_wise(600000, 13, lines)
    point_wise(150000, 20, lines)
    instance(400000, 300, 120, 19, lines)
    whole_step(args.points, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
