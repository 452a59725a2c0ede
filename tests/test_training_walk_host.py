"""The Python layers above the device operators without a GPU: network_blocks.training_walk and the trainable blocks, the decoder and the
head of models/D3Feat.py, kernels/autograd.py's wrappers, KernelPointFCNN.run() / backward() at dropout_prob = 0.5 and
training.MomentumSGD, walked on the CPU over the shared case of tests/training_network_np.py with every entry point of d3feat_amd.ops
they call replaced by its float32 torch statement (the restatements the operator tests pin; the two new backward operators by
tests/pool_grad_np.py).  What is checked is the wiring -- which operator gets which operands, variable names and creation order, the
skip's two consumers, the loss and the optimiser -- against the float64 reference; the kernels are checked on the GPU."""
import numpy as np
import pytest
import torch

import bn_grad_np as bg
import head_grad_np as hg
import kpconv_grad_np as kg
import loss_grad_np as lg
import pool_grad_np as pg
import training_network_np as tn


def _shadow(idx, n):
    return torch.where((idx < 0) | (idx >= n), torch.full_like(idx, n), idx).long()


class _NoContext:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class _Pair:
    loss = "circle_loss"


@pytest.fixture
def torch_operators(monkeypatch):
    """d3feat_amd.ops (and what the wrappers import from it) as float32 torch statements on CPU tensors; -> the list of calls."""
    from d3feat_amd import ops, validation
    from d3feat_amd.kernels import autograd as ag
    calls = []

    def table(nbm, n, *a):
        return tuple(torch.from_numpy(t) for t in pg.transpose_np(nbm.numpy(), n))

    def max_pool_backward(x, inds, y, g, transpose=None, out=None):
        calls.append("ind_max_pool_backward")
        assert transpose is not None and transpose[0].numel() == x.shape[0] + 1
        return torch.from_numpy(pg.max_pool_backward(x.numpy(), inds.numpy(), y.numpy(), g.numpy()).astype(np.float32))

    def upsample_backward(g, inds, N1, C1, transpose=None, out=None):
        calls.append("closest_pool_cat_backward")
        assert transpose is not None and transpose[0].numel() == N1 + 1 and tuple(out.shape) == (N1, C1)
        return out.copy_(torch.from_numpy(pg.upsample_cat_backward(g.numpy(), inds.numpy(), N1, C1)[0].astype(np.float32)))

    def kpconv(q, s, idx, f, KP, W, extent, influence, aggregation):
        return kg.torch_kpconv(q, s, _shadow(idx, s.shape[0]), f, torch.as_tensor(KP), W, extent, influence, aggregation)

    def kpconv_backward(q, s, idx, f, KP, W, g, extent, influence, aggregation, transpose=None, need_features=True, need_weights=True):
        with torch.enable_grad():
            ft, Wt = f.detach().clone().requires_grad_(True), W.detach().clone().requires_grad_(True)
            (kpconv(q, s, idx, ft, KP, Wt, extent, influence, aggregation) * g).sum().backward()
        return (ft.grad if need_features else None), (Wt.grad if need_weights else None)

    def batch_norm_train(x, gamma, beta, eps, residual, leaky, alpha, moving_mean, moving_variance, momentum):
        mean = rstd = None
        if gamma is None:
            z = x + beta
        else:
            z, m, var = bg.torch_batch_norm_training(x, gamma, beta)
            rstd, mean = (var + eps).rsqrt(), torch.stack([m, torch.zeros_like(m)])
            f = float(bg.one_minus(momentum))
            moving_mean.sub_((moving_mean - m) * f)
            moving_variance.sub_((moving_variance - var) * f)
        if residual is not None:
            z = z + residual
        return (torch.nn.functional.leaky_relu(z, alpha) if leaky else z), mean, rstd

    def batch_norm_backward(x, y, g, gamma, mean, rstd, leaky, alpha, need_residual=False):
        g = g * torch.where(y > 0, 1.0, alpha) if leaky else g
        gbeta = g.sum(0)
        if gamma is None:
            return g, None, gbeta, (g if need_residual else None)
        xhat, n = (x - mean[0]) * rstd, x.shape[0]
        gg = (g * xhat).sum(0)
        return gamma * rstd * (g - gbeta / n - xhat * gg / n), gg, gbeta, (g if need_residual else None)

    def head(f, nbm, lens, include_zero, stack_group=0):
        lens = [int(v) for v in lens]
        return hg.torch_head(f, nbm.long(), lens, hg.pad_counts(lens))

    def head_backward(f, nbm, lens, include_zero, gd, gs, stack_group=0, transpose=None):
        calls.append("detect_head_backward")
        with torch.enable_grad():
            ft = f.detach().clone().requires_grad_(True)
            d, s = head(ft, nbm, lens, include_zero)
            ((d * gd).sum() + (s * gs.reshape(s.shape)).sum()).backward()
        return ft.grad

    def loss_gradients(f, s, pts, a, p, **kw):
        calls.append("loss_gradients")
        args = (pts, a.long(), p.long(), kw["safe_radius"], kw["keypts_num"])
        with torch.enable_grad():
            ft, st = f.detach().clone().requires_grad_(True), s.detach().clone().requires_grad_(True)
            total = lg.torch_loss(ft, st.reshape(-1), *args, kw["det_loss_weight"])
            total.backward()
        desc = lg.torch_loss(f.detach(), s.detach().reshape(-1), *args, 0.0)
        r = _Pair()
        r.features, r.scores = ft.grad, st.grad.reshape(-1)
        r.values = torch.tensor([[float(desc), 0.0, float(total.detach() - desc), 0.5, 0.0, 0.0, 0.0, 0.0]])
        r.status = torch.zeros(1, dtype=torch.int32)
        r.figures = lambda p=0: tuple(r.values[p, k] for k in (0, 2, 3, 4, 5))
        return r

    def spied(name, fn):
        def run(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return run
    for name, fn in dict(ind_max_pool=spied("ind_max_pool", lambda x, inds: pg.torch_ind_max_pool(x, inds.numpy())),
                         closest_pool_cat=spied("closest_pool_cat", lambda x, inds, skip=None: pg.torch_closest_pool_cat(x, inds.numpy(), skip)),
                         neighbor_transpose_supports=table, neighbor_transpose=lambda nbm, lens: table(nbm, nbm.shape[0]),
                         ind_max_pool_backward=max_pool_backward, closest_pool_cat_backward=upsample_backward, kpconv_backward=kpconv_backward,
                         batch_norm_train=batch_norm_train, batch_norm_backward=batch_norm_backward, f32_output=_NoContext,
                         gemm=lambda a, b: a @ b, detect_head=head, detect_head_backward=head_backward,
                         unary_backward=lambda x, W, g, need_input=True, need_weights=True: ((g @ W.t()) if need_input else None,
                                                                                           (x.t() @ g) if need_weights else None),
                         as_lens=lambda lens, dev: torch.as_tensor(np.asarray(lens, np.int32))).items():
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(ag, "KPConv_ops", kpconv)
    monkeypatch.setattr(validation, "loss_gradients", loss_gradients)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))     # (the model asks it of the two index lists)
    return calls


def _flat(inp):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    flat = [t(p) for p in inp["points"]] + [t(m) for m in inp["neighbors"]] + [t(m) for m in inp["pools"]] + [t(m) for m in inp["upsamples"]]
    return flat + [t(inp["features"]), t(inp["batch_weights"]), t(inp["in_batches"]), t(inp["out_batches"]), t(inp["stack_lengths"]),
                   t(inp["anc"]), t(inp["pos"]), ["a", "b"], t(inp["points"][0])]


@pytest.mark.parametrize("use_bn", [True, False], ids=["bn", "off"])
def test_training_model_wiring_against_float64(torch_operators, use_bn):
    """Every figure within 1e-4 of the largest entry of the float64 reference (the operators are float32 torch statements here: some
    1e-5 on the gradients of this case, tests/golden/training_network.npz)."""
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    from d3feat_amd.training import MomentumSGD
    cfg, inp, V, ref = tn.config(use_bn), tn.geometry(), tn.variables(use_bn), tn.run(use_bn)
    model = KernelPointFCNN(iter(()), cfg, weights=dict(V), device=torch.device("cpu"))
    with pytest.raises(RuntimeError):
        model.backward()
    model.dropout_prob = 0.5
    d, s = model.run(_flat(inp))
    params = model.backward()
    assert set(model.weights()) == set(V) and set(params) == set(ref["grads"])
    assert np.abs(d.detach().numpy() - ref["desc"]).max() <= 1e-4 and np.abs(s.detach().numpy() - ref["score"]).max() <= 1e-4 * np.abs(ref["score"]).max()
    for name in ("desc_loss", "det_loss", "regularization_loss", "loss"):
        assert abs(float(getattr(model, name).detach()) - ref[name]) <= 1e-4 * abs(ref[name]), name
    for k, p in params.items():
        assert np.abs(p.grad.numpy() - ref["grads"][k]).max() <= 1e-4 * np.abs(ref["grads"][k]).max(), k
    for k, want in ref["moving"].items():
        assert np.abs(model.variables.tensor(k).numpy() - want).max() <= 1e-5 * np.abs(want).max(), k
    L = cfg.num_layers
    for name, count in (("ind_max_pool", L - 1), ("ind_max_pool_backward", L - 1), ("closest_pool_cat", L - 1), ("closest_pool_cat_backward", L - 1),
                        ("detect_head_backward", 1), ("loss_gradients", 1)):
        assert torch_operators.count(name) == count, name
    clip = tn.clip_norm(ref["grads"])
    want, clipped = tn.momentum_step(V, ref["grads"], tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip)
    assert any(clipped.values()) and not all(clipped.values())
    MomentumSGD(model.variables, tn.LEARNING_RATE, tn.SGD_MOMENTUM, clip).step()
    for k, w in want.items():
        assert np.abs(model.variables.tensor(k).numpy() - w).max() <= 1e-5 * max(np.abs(w).max(), tn.LEARNING_RATE * clip), k


def test_without_keypoint_indices_the_skip_tuple_and_the_regularisation_alone(torch_operators):
    from d3feat_amd import validation
    from d3feat_amd.models.KPFCNN_model import KernelPointFCNN
    cfg, inp = tn.config(True), tn.geometry()
    flat = _flat(inp)
    L = cfg.num_layers
    flat[4 * L + 5] = flat[4 * L + 6] = None
    model = KernelPointFCNN(iter(()), cfg, weights=dict(tn.variables(True)), device=torch.device("cpu"))
    model.dropout_prob = 0.5
    model.run(flat)
    assert tuple(float(v) for v in (model.desc_loss, model.det_loss, model.accuracy, model.ave_d_pos, model.ave_d_neg)) == validation.SKIP
    assert "loss_gradients" not in torch_operators and float(model.loss) == float(model.regularization_loss) > 0
    params = model.backward()
    for k, p in params.items():                                     # the gradient of the regularisation: weights_decay * v on the weights
        want = cfg.weights_decay * p.detach() if "weights" in k else torch.zeros_like(p)
        assert torch.allclose(p.grad, want, rtol=1e-6, atol=0), k


def test_direct_block_calls_outside_a_walk_keep_raising(torch_operators):
    from d3feat_amd import ops
    from d3feat_amd.models import network_blocks as nb
    from d3feat_amd.models.variables import VariableStore
    cfg, inp = tn.config(True), tn.geometry()
    f = torch.zeros((len(inp["points"][0]), 16))
    inputs = dict(points=[torch.from_numpy(p) for p in inp["points"]], pools=[torch.from_numpy(m) for m in inp["pools"]])
    up = ops.UpsampleCat(torch.zeros((len(inp["points"][1]), 16)), torch.from_numpy(inp["upsamples"][0]), f)
    with nb.use_variables(VariableStore(seed=1, device=torch.device("cpu"))):
        with pytest.raises(NotImplementedError, match="max pooling"):
            nb.resnetb_strided_block(0, inputs, f, 0.1, 16, cfg, True)
        with pytest.raises(NotImplementedError, match="upsample"):
            nb.unary_block(0, inputs, up, 0.1, 16, cfg, True)
        with nb.training_walk():
            with pytest.raises(NotImplementedError, match="deformable"):
                nb.resnetb_deformable_strided_block(0, inputs, f, 0.1, 16, cfg, True)
            with pytest.raises(NotImplementedError, match="bf16"):
                nb.unary_block(0, inputs, f.to(torch.bfloat16), 0.1, 16, cfg, True)
            out = nb.unary_block(0, inputs, up, 0.1, 16, cfg, True)
            assert tuple(out.shape) == (f.shape[0], 16) and out.requires_grad
    assert nb._TRAINING_WALK == 0
