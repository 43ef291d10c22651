"""The optimizer step on the multi-tensor kernels of csrc/optim.hip.

``build_optimizer(model, optim_cfg, fused=None)`` has the reference's signature
(softgroup/util/optim.py) plus a switch.  Off (the default; ``SG_FUSED_OPTIM=1`` turns it on) it
returns exactly ``getattr(torch.optim, type)(...)``.  On, ``Adam`` / ``AdamW`` / ``SGD`` become
``FusedAdam`` / ``FusedAdamW`` / ``FusedSGD``: subclasses of the torch classes with the same
``param_groups`` and ``state_dict()`` layout whose ``step()`` is one launch per parameter group.

  * AMP: the classes set ``_step_supports_amp_scaling``, so ``scaler.step(optimizer)`` hands over
    ``optimizer.grad_scale`` / ``optimizer.found_inf`` as device tensors; the kernel applies
    ``1 / grad_scale`` and writes nothing when ``found_inf`` is set.  Nothing is read back.
  * ``optimizer.clip_grad_norm = 35.0`` (default None) makes ``step()`` compute the gradient norm
    first (two launches) and apply ``clip_coef`` inside the update.  DIFFERENCE from calling
    ``clip_grad_norm_`` before the step: ``.grad`` itself is left unscaled.  The norm is
    ``optimizer.last_grad_norm`` (a device scalar).
  * ``optimizer.zero_grads_in_step = True`` writes zeros to ``.grad`` after reading it, for callers
    of ``zero_grad(set_to_none=False)``.
  * ``clip_grad_norm_(parameters, max_norm)`` is ``torch.nn.utils.clip_grad_norm_`` in three
    launches without a read-back.

A parameter group takes the stock torch step (bit-identical to the parent class) when its
parameters are on the CPU, when a parameter or gradient is not float32, not contiguous or sparse,
or with ``amsgrad`` / ``maximize`` / ``capturable`` / ``differentiable`` / ``fused``.

The kernels write parameters through raw pointers, which does not bump ``tensor._version``; the
packed-weight and descriptor caches of softgroup_amd.spconv are keyed on it.  Every launched step
therefore ends with ``torch.autograd.graph.increment_version(params)``.
"""
import os

import numpy as np
import torch

from . import _lib as L

ROW_PARAM, ROW_GRAD, ROW_STATE0, ROW_STATE1, ROW_STEP, ROW_COUNT, TABLE_ROWS = range(7)
_RING = 4


def chunk_elems():
    return L.lib().sg_optim_chunk_elems()


def plan_chunks(counts):
    """host int64 [n_chunks, 3] = (tensor, first element, elements) for tensors of `counts` elements"""
    lib = L.lib()
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    n = lib.sg_optim_plan(counts.ctypes.data, len(counts), None, 0)
    if n < 0:
        L.check(int(n), 'sg_optim_plan')
    chunks = np.empty((int(n), 3), dtype=np.int64)
    if n:
        m = lib.sg_optim_plan(counts.ctypes.data, len(counts), chunks.ctypes.data, int(n))
        if m != n:
            L.check(int(m) if m < 0 else -1, 'sg_optim_plan')
    return chunks


def _tensor_ok(t):
    return t.dtype is torch.float32 and t.layout is torch.strided and t.is_contiguous()


class _Plan:
    """Device tables of a fixed list of parameters (and their states): built once, reused while the
    key -- every parameter's data_ptr() -- is unchanged.  The gradient column changes every step
    (zero_grad() drops the buffers, autograd installs fresh ones) and is refilled per step."""

    def __init__(self, key, params, ranges, columns):
        # columns: per tensor (param, state0, state1, step) tensors or None
        self.key, self.params, self.ranges = key, params, ranges
        self.device = dev = params[0].device
        t = len(params)
        host = np.zeros((TABLE_ROWS, t), dtype=np.int64)
        for i, (p, s0, s1, step) in enumerate(columns):
            host[ROW_PARAM, i] = p.data_ptr()
            host[ROW_STATE0, i] = 0 if s0 is None else s0.data_ptr()
            host[ROW_STATE1, i] = 0 if s1 is None else s1.data_ptr()
            host[ROW_STEP, i] = 0 if step is None else step.data_ptr()
            host[ROW_COUNT, i] = p.numel()
        chunks = plan_chunks(host[ROW_COUNT])
        self.n_tensors, self.n_chunks = t, len(chunks)
        # chunk range of every group (chunks are in tensor order)
        starts = [r[0] for r in ranges] + [t]
        first = np.searchsorted(chunks[:, 0], starts) if len(chunks) else np.zeros(len(starts), np.int64)
        self.chunk_ranges = [(int(first[i]), int(first[i + 1])) for i in range(len(ranges))]
        self.table = torch.from_numpy(host).to(dev)
        self.chunks = torch.from_numpy(chunks.reshape(-1)).to(dev) if len(chunks) else None
        self.arrive = torch.zeros(max(t, 1), dtype=torch.int32, device=dev)
        self.ws = L.workspace(L.lib().sg_optim_workspace_bytes(), dev)
        self.keep = columns          # (the table holds raw addresses of these tensors)
        # Staging of the per-step gradient column: a ring of pinned host buffers, each guarded by an
        # event recorded behind its async copy.  A single pinned buffer refilled while the previous
        # step's copy may still be in flight would corrupt the table; a slot is only rewritten after
        # its event has completed (_RING steps later, so the wait is normally free).
        self.ring = [torch.empty(t, dtype=torch.int64).pin_memory() for _ in range(_RING)]
        self.ring_np = [r.numpy() for r in self.ring]
        self.events = [None] * _RING
        self.turn = 0

    def send_grads(self, grad_ptrs):
        i = self.turn
        self.turn = (i + 1) % _RING
        if self.events[i] is None:
            self.events[i] = torch.cuda.Event()
        else:
            self.events[i].synchronize()
        self.ring_np[i][:] = grad_ptrs
        self.table[ROW_GRAD].copy_(self.ring[i], non_blocking=True)
        self.events[i].record()

    def chunk_ptr(self, c0):
        return self.chunks.data_ptr() + 24 * c0


def _norm(plan, grad_scale, max_norm):
    """-> device float [4]: norm, clip_coef, found_inf, 0 (two launches)"""
    if plan.n_chunks == 0:
        return torch.tensor([0.0, 1.0, 0.0, 0.0], device=plan.device)
    out = torch.empty(4, dtype=torch.float32, device=plan.device)
    L.check(L.lib().sg_optim_grad_norm(
        plan.table.data_ptr(), plan.n_tensors, plan.chunks.data_ptr(), plan.n_chunks, L.ptr(grad_scale),
        float(max_norm), out.data_ptr(), plan.ws.data_ptr(), plan.ws.numel(), L.stream()), 'sg_optim_grad_norm')
    return out


def _scalar_f32(t, dev):
    if t is None:
        return None
    if t.dtype is not torch.float32 or t.device != dev:
        t = t.to(device=dev, dtype=torch.float32)
    return t


class _FusedMixin:
    """step() of the fused classes; the concrete class supplies _sg_flags_ok / _sg_states / _sg_launch."""

    def _sg_init(self):
        self._step_supports_amp_scaling = True
        self.clip_grad_norm = None
        self.last_grad_norm = None
        self.zero_grads_in_step = False
        self._sg_plan = None

    # ---- torch layout in and out -----------------------------------------------------------
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._sg_plan = None
        for p, st in self.state.items():
            if p.is_cuda:
                self._sg_after_load(p, st)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._sg_plan = None

    def _sg_parent_step(self, groups):
        """the stock step of the parent class on `groups` only"""
        fn = super().step
        raw = fn.__func__
        if getattr(raw, 'hooked', False):       # (the step hooks already run around our own step())
            raw = raw.__wrapped__
        saved = self.param_groups
        # (the scaler's attributes, handled by step() already; it deletes them itself afterwards)
        amp = {k: self.__dict__.pop(k) for k in ('grad_scale', 'found_inf') if k in self.__dict__}
        self.param_groups = groups
        try:
            raw(self)
        finally:
            self.param_groups = saved
            self.__dict__.update(amp)

    def _sg_group_params(self, group):
        """the parameters of `group` that have a gradient, or None where the group takes the torch step"""
        if not self._sg_flags_ok(group):
            return None
        out = []
        for p in group['params']:
            g = p.grad
            if g is None:
                continue
            if not (p.is_cuda and _tensor_ok(p) and _tensor_ok(g) and g.device == p.device):
                return None
            out.append(p)
        return out

    def _sg_build_plan(self, key, params, ranges, groups):
        columns = []
        for (t0, t1), group in zip(ranges, groups):
            for p in params[t0:t1]:
                col = self._sg_states(p, group)
                if col is None:
                    return None
                columns.append(col)
        return _Plan(key, params, ranges, columns)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, 'grad_scale', None), getattr(self, 'found_inf', None)
        clip = self.clip_grad_norm

        fused_groups, stock_groups, params, ranges = [], [], [], []
        device = None
        for group in self.param_groups:
            ps = self._sg_group_params(group)
            if ps is not None and ps and device is not None and ps[0].device != device:
                ps = None                        # (one device per optimizer on the fused path)
            if ps is None:
                stock_groups.append(group)
            elif ps:
                device = ps[0].device
                ranges.append((len(params), len(params) + len(ps)))
                params += ps
                fused_groups.append(group)

        plan = None
        if params:
            key = (tuple(p.data_ptr() for p in params), tuple(ranges))
            plan = self._sg_plan
            if plan is None or plan.key != key:
                plan = self._sg_plan = self._sg_build_plan(key, params, ranges, fused_groups)
            if plan is None:                     # (a state tensor the kernels cannot take)
                stock_groups, fused_groups = list(self.param_groups), []

        if stock_groups and (grad_scale is not None or found_inf is not None or clip is not None):
            # The torch step knows neither the scaler's tensors nor the fused-in clip: do on the host what
            # GradScaler and clip_grad_norm_ would have done, for all groups alike.
            if found_inf is not None and bool(found_inf.item()):
                return loss
            every = [p for g in self.param_groups for p in g['params'] if p.grad is not None]
            if grad_scale is not None:
                inv = grad_scale.double().reciprocal().float()
                for p in every:
                    p.grad.mul_(inv.to(p.grad.device))
            if clip is not None:
                self.last_grad_norm = torch.nn.utils.clip_grad_norm_(every, clip)
            grad_scale = found_inf = clip = None

        if fused_groups:
            with torch.cuda.device(plan.device):
                grad_scale = _scalar_f32(grad_scale, plan.device)
                found_inf = _scalar_f32(found_inf, plan.device)
                plan.send_grads([p.grad.data_ptr() for p in params])
                coef = None
                if clip is not None:
                    out = _norm(plan, grad_scale, clip)
                    self.last_grad_norm, coef = out[0], out[1]
                if plan.n_chunks:
                    for group, (c0, c1) in zip(fused_groups, plan.chunk_ranges):
                        if c1 > c0:
                            self._sg_launch(plan, group, c0, c1 - c0, grad_scale, found_inf, coef)
                # Raw-pointer writes do not bump _version; the packed-weight / descriptor caches of
                # softgroup_amd.spconv are keyed on it.  (A skipped step bumps too: one re-pack.)
                torch.autograd.graph.increment_version(params)
                if self.zero_grads_in_step:
                    torch.autograd.graph.increment_version([p.grad for p in params])
        if stock_groups:
            self._sg_parent_step(stock_groups)
        return loss


def _device_step(st, p, default=0.0):
    step = st.get('step')
    if step is None:
        step = torch.full((), default, dtype=torch.float32, device=p.device)
    elif not (torch.is_tensor(step) and step.device == p.device and step.dtype is torch.float32 and step.dim() == 0):
        step = torch.as_tensor(step, dtype=torch.float32).reshape(()).to(p.device)
    st['step'] = step
    return step


def _host_steps(states):
    """{index: step as a CPU float32 scalar} with one device-to-host copy"""
    dev = {k: st['step'] for k, st in states.items() if torch.is_tensor(st.get('step')) and st['step'].is_cuda}
    if not dev:
        return {}
    host = torch.stack([s.reshape(()).float() for s in dev.values()]).cpu()
    return {k: host[i].clone() for i, k in enumerate(dev)}


class _FusedAdamMixin(_FusedMixin):
    _sg_adamw = False

    def _sg_flags_ok(self, group):
        return not (group.get('amsgrad') or group.get('maximize') or group.get('capturable')
                    or group.get('differentiable') or group.get('fused')
                    or torch.is_tensor(group['lr']) or any(torch.is_tensor(b) for b in group['betas']))

    def _sg_after_load(self, p, st):
        if 'step' in st:
            _device_step(st, p)

    def _sg_states(self, p, group):
        st = self.state[p]
        if 'exp_avg' not in st:
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        m, v = st['exp_avg'], st['exp_avg_sq']
        for s in (m, v):
            if not (s.device == p.device and _tensor_ok(s) and s.numel() == p.numel()):
                return None
        return p, m, v, _device_step(st, p)

    def _sg_launch(self, plan, group, c0, n, grad_scale, found_inf, coef):
        b1, b2 = group['betas']
        L.check(L.lib().sg_optim_adam_step(
            plan.table.data_ptr(), plan.n_tensors, plan.chunk_ptr(c0), n, float(group['lr']), float(b1), float(b2),
            float(group['eps']), float(group['weight_decay']),
            int(bool(group.get('decoupled_weight_decay', self._sg_adamw))), L.ptr(grad_scale),
            L.ptr(found_inf), L.ptr(coef), int(self.zero_grads_in_step), plan.arrive.data_ptr(), L.stream()),
            'sg_optim_adam_step')

    def state_dict(self):
        """torch's layout; `step` as the CPU float32 scalar the stock class keeps"""
        sd = super().state_dict()
        host = _host_steps(sd['state'])
        sd['state'] = {k: ({**st, 'step': host[k]} if k in host else st) for k, st in sd['state'].items()}
        return sd


class FusedAdam(_FusedAdamMixin, torch.optim.Adam):

    def __init__(self, params, *args, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._sg_init()


class FusedAdamW(_FusedAdamMixin, torch.optim.AdamW):
    _sg_adamw = True

    def __init__(self, params, *args, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._sg_init()


class FusedSGD(_FusedMixin, torch.optim.SGD):
    """torch.optim.SGD keeps no step counter; the fused step keeps one per tensor (state['step'], a
    device scalar) to know torch's "first step", where the momentum buffer starts as the gradient.
    state_dict() drops it, and a momentum buffer that has not seen a step, again: torch's layout."""

    def __init__(self, params, *args, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._sg_init()

    def _sg_flags_ok(self, group):
        return not (group.get('maximize') or group.get('differentiable') or group.get('fused')
                    or torch.is_tensor(group['lr']))

    def _sg_after_load(self, p, st):
        _device_step(st, p, default=1.0 if st.get('momentum_buffer') is not None else 0.0)

    def _sg_states(self, p, group):
        st = self.state[p]
        buf = st.get('momentum_buffer')
        step = _device_step(st, p, default=0.0 if buf is None else 1.0)
        if group['momentum'] == 0:
            return p, None, None, step
        if buf is None:
            # (no step seen: the kernel sets it to the gradient; a counter that says otherwise is reset)
            buf = st['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            step.zero_()
        if not (buf.device == p.device and _tensor_ok(buf) and buf.numel() == p.numel()):
            return None
        return p, buf, None, step

    def _sg_parent_step(self, groups):
        super()._sg_parent_step(groups)
        # the torch step has created or advanced the momentum buffers: no longer a first step
        for g in groups:
            for p in g['params']:
                st = self.state.get(p)
                if st and torch.is_tensor(st.get('step')) and st.get('momentum_buffer') is not None:
                    st['step'].fill_(1.0)

    def _sg_launch(self, plan, group, c0, n, grad_scale, found_inf, coef):
        L.check(L.lib().sg_optim_sgd_step(
            plan.table.data_ptr(), plan.n_tensors, plan.chunk_ptr(c0), n, float(group['lr']),
            float(group['momentum']), float(group['dampening']), float(group['weight_decay']),
            int(bool(group['nesterov'])), L.ptr(grad_scale), L.ptr(found_inf), L.ptr(coef),
            int(self.zero_grads_in_step), plan.arrive.data_ptr(), L.stream()), 'sg_optim_sgd_step')

    def state_dict(self):
        sd = super().state_dict()
        host = _host_steps(sd['state'])
        state = {}
        for k, st in sd['state'].items():
            st = dict(st)
            st.pop('step', None)
            if k in host and float(host[k]) == 0.0:
                st['momentum_buffer'] = None
            state[k] = st
        sd['state'] = state
        return sd


FUSED_CLASSES = {'Adam': FusedAdam, 'AdamW': FusedAdamW, 'SGD': FusedSGD}


def build_optimizer(model, optim_cfg, fused=None):
    """The reference's build_optimizer; with `fused` (None: the environment's SG_FUSED_OPTIM=1; default
    off) Adam / AdamW / SGD come from the fused classes, any other type from torch.optim unchanged."""
    assert 'type' in optim_cfg
    _optim_cfg = optim_cfg.copy()
    optim_type = _optim_cfg.pop('type')
    if fused is None:
        fused = os.environ.get('SG_FUSED_OPTIM', '0') == '1'
    optim = FUSED_CLASSES.get(optim_type) if fused else None
    if optim is None:
        optim = getattr(torch.optim, optim_type)
    return optim(filter(lambda p: p.requires_grad, model.parameters()), **_optim_cfg)


_clip_plans = {}      # key -> _Plan of the stand-alone clip_grad_norm_ (a few parameter lists at most)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ (same signature, same return value: the total norm as a device
    scalar) as norm + scale: three launches, no read-back.  A norm_type other than 2, CPU tensors and
    gradients that are not contiguous float32 go to torch."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    ok = float(norm_type) == 2.0 and bool(params) and float(max_norm) >= 0.0
    if ok:
        dev = params[0].device
        ok = dev.type == 'cuda' and all(p.grad.device == dev and _tensor_ok(p.grad) for p in params)
    if not ok:
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type, error_if_nonfinite, foreach)
    key = tuple((p.data_ptr(), p.numel()) for p in params)
    plan = _clip_plans.get(key)
    if plan is None:
        if len(_clip_plans) >= 4:
            _clip_plans.clear()
        plan = _clip_plans[key] = _Plan(key, params, [(0, len(params))], [(p, None, None, None) for p in params])
    grads = [p.grad for p in params]
    with torch.cuda.device(dev):
        plan.send_grads([g.data_ptr() for g in grads])
        out = _norm(plan, None, max_norm)
        if error_if_nonfinite and bool(out[2].item()):
            raise RuntimeError('The total norm for gradients from `parameters` is non-finite, so it cannot be clipped.')
        if plan.n_chunks:
            L.check(L.lib().sg_optim_scale_grads(plan.table.data_ptr(), plan.n_tensors, plan.chunks.data_ptr(),
                                                 plan.n_chunks, out[1:].data_ptr(), L.stream()), 'sg_optim_scale_grads')
            torch.autograd.graph.increment_version(grads)
    return out[0]
