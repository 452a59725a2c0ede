"""The optimiser's update of the reference's trainer (utils/trainer.py:119-156): tf.train.MomentumOptimizer behind a per-variable
tf.clip_by_norm, applied in place on the parameter leaves of a VariableStore.

    opt = MomentumSGD(model.variables, learning_rate, momentum, grad_clip_norm)
    model.dropout_prob = 0.5; model.run(flat_inputs); model.backward(); opt.step()

Per variable:  g <- g * clip / max(|g|_2, clip)  (grad_clip_norm > 0),  accum <- momentum * accum + g,  var <- var - lr * accum.

MomentumSGD writes this with torch operations, five or six small kernels for each of about a hundred tensors: the statement the device
call is held against, a third of a training step's time (tools/training_step_bench.py).  DeviceMomentumSGD is the hot path: the same
update of every variable in ONE call of two launches (ops.momentum_sgd_step, d3f_momentum_sgd in include/d3feat_amd.h), with the
hyper-parameters read on the device, the weight decay of the regularisation loss folded in, and optionally gradient buffers that stay in
place -- what a captured training step needs.

    opt = DeviceMomentumSGD(model.variables, learning_rate, momentum, grad_clip_norm, weights_decay=config.weights_decay,
                            persistent_grads=True)
    opt.attach(model)                         # fold_regularization: the decay's gradient and the loss's value come from the step
    model.run(flat_inputs); model.backward(keep_grads=True); opt.step()

The two classes differ in roundings only (include/d3feat_amd.h has the device call's): torch's p.add_(a, alpha=-lr) is a fused
multiply-add on the CPU, where the device call rounds lr * a' on its own, and torch's float32 vector_norm is off the float64 norm by
about 6e-7 relative on 1e5 entries, where the device call adds the squares in float64.  tests/optimizer_np.py restates the device call
bit for bit.
"""
import numpy as np
import torch


class MomentumSGD:
    def __init__(self, store, learning_rate, momentum=0.98, grad_clip_norm=100.0):
        self.store = store
        self.learning_rate, self.momentum, self.grad_clip_norm = float(learning_rate), float(momentum), float(grad_clip_norm)
        self.accum = {}          # name -> the variable's `Momentum` slot (zeros at creation)

    @torch.no_grad()
    def step(self, commit=False):
        """One update of every parameter that has a .grad; commit: store.commit() afterwards (the host masters and the folded copies
        of the inference path follow).  -> the names updated."""
        done = []
        for name, p in self.store.parameters().items():
            g = p.grad
            if g is None:
                continue
            if self.grad_clip_norm > 0:                      # (the norm stays on the device: no copy, no read-back)
                g = g * (self.grad_clip_norm / torch.linalg.vector_norm(g).clamp_min(self.grad_clip_norm))
            a = self.accum.get(name)
            if a is None:
                a = self.accum[name] = torch.zeros_like(p)
            a.mul_(self.momentum).add_(g)
            p.add_(a, alpha=-self.learning_rate)
            done.append(name)
        if commit:
            self.store.commit()
        return done


def _round_up(n, to):
    return (n + to - 1) // to * to


class DeviceMomentumSGD:
    """MomentumSGD's interface -- step(commit=False) -> names, .accum (name -> tensor) -- over one device call.

    accum: views of ONE arena, every offset rounded up to 64 elements.  persistent_grads: every leaf's .grad is installed as a zeroed
    view of a second arena, and the step zeroes the gradients it has used; with KernelPointFCNN.backward(keep_grads=True) autograd then
    accumulates in place and no gradient address ever changes.  weights_decay > 0 decays exactly the variables whose name contains
    `weights` (KPFCNN_model.py:189-191) and regularization_loss, a device scalar, holds float(weights_decay * sum 0.5 |v|^2) of the
    values BEFORE the last step -- the regularisation loss that belongs to the forward pass the step's gradients came from.

    The descriptor table (addresses, counts, decay flags) is rebuilt on the host at every step and uploaded -- one small pinned
    asynchronous copy -- only when an entry changed.  A step inside a stream capture must find it unchanged: step once eagerly first.
    After the kernels have written the device copies, every updated leaf's version counter is bumped, which the packed weight copies of
    d3feat_amd.ops are keyed on; a REPLAYED capture does not run that host code: call mark_updated() after replays, before the
    inference forms read the weights.  Not built: a device-side commit() (it goes through the host), deformable blocks and the 0.1
    scale of offset_conv gradients, bf16."""
    PAD = 64

    def __init__(self, store, learning_rate, momentum=0.98, grad_clip_norm=100.0, weights_decay=0.0, persistent_grads=False):
        self.store = store
        self.learning_rate, self.momentum, self.grad_clip_norm = float(learning_rate), float(momentum), float(grad_clip_norm)
        self.weights_decay, self.persistent_grads = float(weights_decay), bool(persistent_grads)
        self.accum = {}
        self.hyper = self.regularization_loss = None
        if store.device is not None:
            self._scalars(torch.device(store.device))
        self._names = None
        self._uploaded = None         # the table the device holds (host copy)
        self._copied = None           # event behind the last upload: the pinned buffer is free again after it

    # ---- layout ---------------------------------------------------------------------------------------
    def _scalars(self, device):
        """The device scalars, made once: captured steps read them by address."""
        self.hyper = torch.tensor([self.learning_rate, self.momentum, self.grad_clip_norm, self.weights_decay], dtype=torch.float32,
                                  device=device)
        self._reg = torch.zeros(1, dtype=torch.float32, device=device)
        self.regularization_loss = self._reg[0]

    def _arena(self, params, device):
        """-> (arena, {name: view shaped like the parameter}), offsets rounded up to PAD elements, zeros."""
        offs, total = {}, 0
        for name, p in params.items():
            offs[name] = total
            total = _round_up(total + p.numel(), self.PAD)
        arena = torch.zeros(max(total, self.PAD), dtype=torch.float32, device=device)
        return arena, {name: arena[o:o + params[name].numel()].view(params[name].shape) for name, o in offs.items()}

    def _layout(self, params):
        from . import ops
        names = list(params)
        device = self.store.device if self.store.device is not None else next(iter(params.values())).device
        device = torch.device(device)
        for name, p in params.items():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("DeviceMomentumSGD: %s must be a contiguous float32 tensor" % name)
        old = self.accum
        self.accum_arena, self.accum = self._arena(params, device)
        for name, a in old.items():                                   # (variables created since the last step join with zeros)
            if name in self.accum:
                self.accum[name].copy_(a)
        if self.persistent_grads:
            self.grad_arena, self.grads = self._arena(params, device)
            for name, p in params.items():
                if p.grad is not None:
                    self.grads[name].copy_(p.grad)
                p.grad = self.grads[name]
        self._names = names
        self._counts = np.array([params[n].numel() for n in names], np.int64)
        self._decay = np.array([1 if (self.weights_decay > 0 and "weights" in n) else 0 for n in names], np.int64)
        T = len(names)
        if self.hyper is None:
            self._scalars(device)
        self._uploaded = None
        if device.type != "cuda":
            return                                                    # (a host store: the update itself is _launch's, see there)
        table = ops.momentum_sgd_plan(self._counts)
        self._chunks = torch.from_numpy(table).to(device)
        self._desc = torch.zeros((T, 4), dtype=torch.int64, device=device)
        self._pinned = torch.zeros((T, 4), dtype=torch.int64).pin_memory()
        self._ws = torch.empty(max(ops.momentum_sgd_workspace_bytes(T, table.shape[0]), 1), dtype=torch.uint8, device=device)

    def set_learning_rate(self, learning_rate):
        """The device scalar a step reads: a captured step follows the trainer's decays without a new capture."""
        self.learning_rate = float(learning_rate)
        if self.hyper is not None:
            self.hyper[0:1].fill_(self.learning_rate)

    def attach(self, model):
        """Fold the regularisation term of `model` (a KernelPointFCNN) into this optimiser: model.fold_regularization = True and
        model.regularization_loss becomes this optimiser's device scalar."""
        model.fold_regularization = True
        model.regularization_scalar = self
        return self

    # ---- the step ---------------------------------------------------------------------------------------
    def _table(self, params):
        """The descriptor table of this step on the host -> (i64[T, 4], the live names)."""
        table = np.zeros((len(self._names), 4), np.int64)
        live = []
        for i, name in enumerate(self._names):
            p, g = params[name], params[name].grad
            table[i, 0], table[i, 2] = p.data_ptr(), self.accum[name].data_ptr()
            table[i, 3] = self._counts[i] + (self._decay[i] << 32)
            if g is None:
                continue
            if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                raise ValueError("DeviceMomentumSGD: the gradient of %s must be a contiguous float32 tensor beside it" % name)
            table[i, 1] = g.data_ptr()
            live.append(name)
        return table, live

    def _launch(self, params, table, live):
        """The device call.  (tests/test_optimizer_host.py replaces this by the numpy restatement on a host store.)"""
        from . import ops
        if self._uploaded is None or not np.array_equal(table, self._uploaded):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceMomentumSGD.step(): a gradient address changed inside a stream capture; use persistent_grads "
                                   "and step once eagerly before capturing")
            if self._copied is not None:
                self._copied.synchronize()
            self._pinned.copy_(torch.from_numpy(table))
            self._desc.copy_(self._pinned, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record(torch.cuda.current_stream(self._desc.device))
            self._uploaded = table
        ops.momentum_sgd_step(self._desc, self._chunks, self.hyper, zero_grad=self.persistent_grads, reg_loss=self._reg, ws=self._ws)

    def mark_updated(self, names=None):
        """Bump the version counter of the updated leaves (the device copies share it): the packed weight copies of d3feat_amd.ops are
        keyed on it, and a kernel's write does not move it."""
        params = self.store.parameters()
        for name in (self._names if names is None else names):
            torch.autograd.graph.increment_version(params[name])

    @torch.no_grad()
    def step(self, commit=False):
        """One update of every parameter that has a .grad, in one device call; commit: store.commit() afterwards.  -> the names
        updated."""
        params = self.store.parameters()
        if not params:
            return []
        if self._names != list(params):
            self._layout(params)
        table, live = self._table(params)
        self._launch(params, table, live)
        self.mark_updated(live)
        if commit:
            self.store.commit()
        return live
