"""The optimiser's update of the reference's trainer (utils/trainer.py:119-156): tf.train.MomentumOptimizer behind a per-variable
tf.clip_by_norm, applied in place on the parameter leaves of a VariableStore.

    opt = MomentumSGD(model.variables, learning_rate, momentum, grad_clip_norm)
    model.dropout_prob = 0.5; model.run(flat_inputs); model.backward(); opt.step()

Per variable:  g <- g * clip / max(|g|_2, clip)  (grad_clip_norm > 0),  accum <- momentum * accum + g,  var <- var - lr * accum.
About a hundred small tensors, written with torch operations: not the hot path (tools/training_step_bench.py times it).
"""
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
