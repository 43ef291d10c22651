"""The optimizer step alone and inside a training step: torch.optim.Adam (default), torch.optim.Adam
(fused=True), softgroup_amd.optim.FusedAdam, and FusedAdam with clip_grad_norm=35 against torch's
clip_grad_norm_ + step, in one run, on the parameter set of the full S3DIS-section model that
tools/train_step_profile.py builds (random gradients).  Medians of 20 steps after 5 warm-up steps: host
time per step() call and device time from events.  Then one whole training step (forward + backward +
step) with the switch off and on.
Usage (GPU box): python tools/optim_bench.py [points] [out.txt]      default 100000 profiles/optim_bench.txt"""
import copy
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from softgroup_amd import optim as O  # noqa: E402
from softgroup_amd import synthetic  # noqa: E402
from softgroup_amd.model import SoftGroup  # noqa: E402

WARMUP, STEPS = 5, 20


def median(xs):
    return sorted(xs)[len(xs) // 2]


def build(n):
    cfg = copy.deepcopy(synthetic.S3DIS_MODEL_CFG)
    cfg['test_cfg']['x4_split'] = False
    cfg['fixed_modules'] = []
    xyz, rgb, inst = synthetic.scene_s2(seed=21, n=n)
    batch = synthetic.make_batch(xyz, rgb, instance_labels=inst)
    batch['semantic_labels'] = batch['semantic_labels'].clamp(max=12)
    batch['instance_cls'] = batch['instance_cls'].clamp(max=12)
    torch.manual_seed(0)
    model = SoftGroup(**cfg).cuda()
    with torch.no_grad():
        model.semantic_linear[-1].weight.normal_(0, 20.0)
    model.train()
    return model, batch


def bench_step(make, shapes, before=None):
    """-> (host ms, device ms) of opt.step() (with `before`, e.g. a clip, inside the timed region)"""
    params = [torch.randn(s, device='cuda').mul_(0.1).requires_grad_(True) for s in shapes]
    opt = make(params)
    host, dev = [], []
    for it in range(WARMUP + STEPS):
        for p in params:                       # fresh buffers every step, as autograd installs them
            p.grad = torch.randn_like(p)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        if before is not None:
            before(params)
        opt.step()
        t1 = time.perf_counter()
        b.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            host.append((t1 - t0) * 1e3)
            dev.append(a.elapsed_time(b))
        opt.zero_grad()
    return median(host), median(dev)


def bench_train(model, batch, start, fused):
    model.load_state_dict(start)
    opt = O.build_optimizer(model, dict(type='Adam', lr=1e-4), fused=fused)
    ts = []
    for it in range(3 + 8):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss, _ = model(batch, return_loss=True)
        opt.zero_grad()
        loss.backward()
        t1 = time.perf_counter()
        opt.step()
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if it >= 3:
            ts.append(((t2 - t1) * 1e3, (t3 - t0) * 1e3))
    return median([t[0] for t in ts]), median([t[1] for t in ts])


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'optim_bench.txt')
    model, batch = build(n)
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    total = sum(torch.Size(s).numel() for s in shapes)
    lines = [f'# tools/optim_bench.py {n}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'# {len(shapes)} parameter tensors, {total} elements; medians of {STEPS} steps after {WARMUP} warm-up',
             '', f'{"optimizer step":<48s} {"host ms":>9s} {"device ms":>10s}']

    def clip(params):
        torch.nn.utils.clip_grad_norm_(params, 35.0)

    def fused_clip(params):
        opt = O.FusedAdam(params, lr=1e-4)
        opt.clip_grad_norm = 35.0
        return opt

    rows = [('torch.optim.Adam (default)', lambda ps: torch.optim.Adam(ps, lr=1e-4), None),
            ('torch.optim.Adam(fused=True)', lambda ps: torch.optim.Adam(ps, lr=1e-4, fused=True), None),
            ('FusedAdam', lambda ps: O.FusedAdam(ps, lr=1e-4), None),
            ('clip_grad_norm_(35) + torch.optim.Adam', lambda ps: torch.optim.Adam(ps, lr=1e-4), clip),
            ('clip_grad_norm_(35) + torch.optim.Adam(fused=True)',
             lambda ps: torch.optim.Adam(ps, lr=1e-4, fused=True), clip),
            ('FusedAdam, clip_grad_norm = 35', fused_clip, None)]
    for name, make, before in rows:
        h, d = bench_step(make, shapes, before)
        lines.append(f'{name:<48s} {h:9.3f} {d:10.3f}')
        print(lines[-1], flush=True)
    lines += ['', f'{"training step (forward + backward + step)":<48s} {"step() ms":>9s} {"whole ms":>10s}']
    start = copy.deepcopy(model.state_dict())
    for name, fused in (('SG_FUSED_OPTIM off (torch.optim.Adam)', False), ('SG_FUSED_OPTIM on (FusedAdam)', True)):
        h, w = bench_train(model, batch, start, fused)
        lines.append(f'{name:<48s} {h:9.3f} {w:10.3f}')
        print(lines[-1], flush=True)
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
