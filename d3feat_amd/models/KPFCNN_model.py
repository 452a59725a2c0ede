"""KernelPointFCNN: the model class of the reference (models/KPFCNN_model.py:49-203): inference, and the training-mode forward with
its loss under torch.autograd.

    model = KernelPointFCNN(flat_inputs, config)          # same constructor signature
    model.anchor_inputs / out_features / out_scores / anc_id / pos_id / dropout_prob

`flat_inputs` is the positional list built by datasets/common.py:1410-1413 + the dataset tail
(datasets/ThreeDMatch.py:322; unpacked at KPFCNN_model.py:86-121), either as a list of tensors (the network is
evaluated immediately) or an iterator of such lists (dataset.flat_inputs; `run()` pulls the next element, which is
what one sess.run does in the reference).  Weights: a dict keyed by the checkpoint variable names (without the
`KernelPointNetwork/` root); missing variables are created like the reference's initialisers.

Of the loss graph (:143-191) the forward figures a validation fetches are here: after run() the attributes desc_loss, det_loss,
accuracy, ave_d_pos, ave_d_neg are device scalars (d3feat_amd/validation.py, one pair; safe_radius, keypts_num and det_loss_weight
from the config), the skip tuple (0, 0, -1, 0, 0) when flat_inputs carries no keypoint indices.

Training: with model.dropout_prob < 0.99 (the reference feeds 0.5, utils/trainer.py:270) run() walks the architecture in training mode
(batch statistics, moving statistics updated in place, every operator under torch.autograd: kernels/autograd.py), takes the five figures
and the gradients of desc_loss + det_loss from ONE validation.loss_gradients call, and sets regularization_loss = weights_decay * the sum
of 0.5 |v|^2 over the variables whose name contains `weights` (:189-190) and loss = desc_loss + det_loss + regularization_loss (:191),
an autograd scalar.  backward() zeroes the .grad of variables.parameters() and calls loss.backward(); d3feat_amd/training.py holds the
optimiser's update.  With fold_regularization = True the regularisation term stays out of the graph (loss = desc_loss + det_loss): its
gradient weights_decay * v is added by training.DeviceMomentumSGD's step, and regularization_loss is that optimiser's device scalar --
the figure of the PREVIOUS step until step() has run on this pass's gradients.  Under the skip rule (:172-186) the five figures are the skip tuple and carry no gradient.  Deformable blocks,
bf16 feature rows, graph replay and several GPUs are not built for training.
"""
import numpy as np
import torch

from .. import validation
from ..kernels.autograd import pair_loss_trainable
from .D3Feat import assemble_FCNN_blocks
from .network_blocks import use_variables
from .variables import VariableStore


class KernelPointFCNN:
    def __init__(self, flat_inputs, config, weights=None, seed=42, device=None):
        self.config = config
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = device
        self.variables = VariableStore(weights, seed=seed, device=device)
        self.dropout_prob = 1.0          # inference (a tf.placeholder fed with 1.0 in the reference)
        self.flat_inputs = flat_inputs
        self.anchor_inputs = None
        self.out_features = self.out_scores = None
        self.anc_id = self.pos_id = None
        self.anc_keypts_inds = self.pos_keypts_inds = None
        self.validation = None
        # the tuple of KPFCNN_model.py:179-184, made once: a run without keypoint indices adds no launch
        self._skip = None
        self.desc_loss = self.det_loss = self.accuracy = self.ave_d_pos = self.ave_d_neg = None
        self.regularization_loss = self.loss = None
        # True: the regularisation term stays out of the autograd graph (loss = desc_loss + det_loss); its gradient and its value
        # come from a training.DeviceMomentumSGD built with weights_decay (its attach(model) sets both attributes)
        self.fold_regularization = False
        self.regularization_scalar = None
        if isinstance(flat_inputs, (list, tuple)):
            self.run(flat_inputs)

    def unpack(self, flat_inputs):
        """KPFCNN_model.py:86-121."""
        L = self.config.num_layers
        a = dict()
        a['points'] = flat_inputs[:L]
        a['neighbors'] = flat_inputs[L:2 * L]
        a['pools'] = flat_inputs[2 * L:3 * L]
        a['upsamples'] = flat_inputs[3 * L:4 * L]
        ind = 4 * L
        a['features'] = flat_inputs[ind]; ind += 1
        a['batch_weights'] = flat_inputs[ind]; ind += 1
        a['in_batches'] = flat_inputs[ind]; ind += 1
        a['out_batches'] = flat_inputs[ind]; ind += 1
        a['stack_lengths'] = flat_inputs[ind]; ind += 1
        self.anc_keypts_inds = flat_inputs[ind]; ind += 1
        self.pos_keypts_inds = flat_inputs[ind]; ind += 1
        ids = flat_inputs[ind]
        self.anc_id, self.pos_id = ids[0], ids[1]
        ind += 1
        a['backup_points'] = flat_inputs[ind]
        if self.config.dataset == 'KITTI' and len(flat_inputs) > ind + 1:
            ind += 1
            a['trans'] = flat_inputs[ind]
        return a

    def run(self, flat_inputs=None):
        """One forward pass = sess.run([out_features, out_scores], {dropout_prob: 1.0}) (utils/tester.py:198-199); with
        dropout_prob < 0.99 the training-mode forward and the loss of :143-191 (backward() follows)."""
        if flat_inputs is None:
            flat_inputs = next(self.flat_inputs) if not isinstance(self.flat_inputs, (list, tuple)) else self.flat_inputs
        self.anchor_inputs = self.unpack(flat_inputs)
        with use_variables(self.variables):
            with self.variables.variable_scope('KernelPointNetwork'):
                pass
            self.out_features, self.out_scores = assemble_FCNN_blocks(self.anchor_inputs, self.config, self.dropout_prob)
        if self.dropout_prob < 0.99:
            self._training_loss()
        else:
            self.regularization_loss = self.loss = None
            self._validation_figures()
        return self.out_features, self.out_scores

    def _keypoint_indices(self):
        """The two index lists as int32 device vectors, or (None, None): "no indices"."""
        anc, pos = self.anc_keypts_inds, self.pos_keypts_inds
        if isinstance(anc, np.ndarray) and isinstance(pos, np.ndarray) and anc.size > 0:     # as a dataset generator yields them
            anc = torch.from_numpy(np.ascontiguousarray(anc.reshape(-1), dtype=np.int32)).to(self.device)
            pos = torch.from_numpy(np.ascontiguousarray(pos.reshape(-1), dtype=np.int32)).to(self.device)
        if not (isinstance(anc, torch.Tensor) and isinstance(pos, torch.Tensor) and anc.is_cuda and pos.is_cuda):
            return None, None
        return anc.reshape(-1).to(torch.int32), pos.reshape(-1).to(torch.int32)

    def _training_loss(self):
        """KPFCNN_model.py:143-191 on the training-mode outputs: the figures and the gradients of ONE loss_gradients call, the
        regularisation loss in plain torch on the parameter leaves, and their sum."""
        cfg = self.config
        anc, pos = self._keypoint_indices()
        pair = 0.0
        if anc is None:
            if self._skip is None:
                self._skip = torch.tensor(validation.SKIP, dtype=torch.float32, device=self.device)
            self.validation = None
            self.desc_loss, self.det_loss, self.accuracy, self.ave_d_pos, self.ave_d_neg = self._skip.unbind(0)
        else:
            pair, self.validation = pair_loss_trainable(
                self.out_features, self.out_scores, self.anchor_inputs['backup_points'], anc, pos, safe_radius=cfg.safe_radius,
                keypts_num=cfg.keypts_num, det_loss_weight=cfg.det_loss_weight)
            self.desc_loss, self.det_loss, self.accuracy, self.ave_d_pos, self.ave_d_neg = self.validation.figures(0)
        if self.fold_regularization:
            # the optimiser's device scalar: float(weights_decay * sum 0.5 |v|^2) of the values the LAST step started from, so it is the
            # previous step's figure until step() has run on this pass's gradients, and this pass's afterwards
            opt = self.regularization_scalar
            self.regularization_loss = opt.regularization_loss if opt is not None else None
            self.loss = pair if isinstance(pair, torch.Tensor) else torch.zeros((), dtype=torch.float32, device=self.device)
            return
        reg = [0.5 * (p * p).sum() for name, p in self.variables.parameters().items() if 'weights' in name]
        self.regularization_loss = float(cfg.weights_decay) * torch.stack(reg).sum()
        self.loss = pair + self.regularization_loss

    def backward(self, keep_grads=False):
        """The gradient of `loss` into the .grad of every leaf of variables.parameters() (zeroed first) -> that dict.
        keep_grads: the .grad tensors stay where they are and autograd accumulates into them in place -- for gradient buffers that an
        optimiser has installed and zeroes itself (training.DeviceMomentumSGD, persistent_grads); a leaf the backward does not reach
        keeps its zeros."""
        if self.loss is None:
            raise RuntimeError('backward(): run() with dropout_prob < 0.99 first')
        params = self.variables.parameters()
        if not keep_grads:
            for p in params.values():
                p.grad = None
        if self.loss.requires_grad:                      # (folded regularisation under the skip rule: nothing carries a gradient)
            self.loss.backward()
        for p in params.values():
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        return params

    def _validation_figures(self):
        """KPFCNN_model.py:131-186, forward: desc_loss (the circle loss), det_loss, accuracy, ave_d_pos, ave_d_neg of the pair just
        run, as device scalars."""
        # keypoint indices are DEVICE tensors (or what a generator yields); anything else in these two slots -- None, the empty
        # arrays of the test generators, a host placeholder -- is "no indices": the skip tuple, and no launch
        anc, pos = self._keypoint_indices()
        if anc is None:
            if self._skip is None:
                self._skip = torch.tensor(validation.SKIP, dtype=torch.float32, device=self.device)
            self.validation = None
            self.desc_loss, self.det_loss, self.accuracy, self.ave_d_pos, self.ave_d_neg = self._skip.unbind(0)
            return
        cfg = self.config
        self.validation = validation.validation_pairs(
            self.out_features, self.out_scores, self.anchor_inputs['backup_points'], anc, pos, safe_radius=cfg.safe_radius, keypts_num=cfg.keypts_num,
            det_loss_weight=cfg.det_loss_weight)
        self.desc_loss, self.det_loss, self.accuracy, self.ave_d_pos, self.ave_d_neg = self.validation.figures(0)

    __call__ = run

    def weights(self):
        """All variables (numpy), keyed by checkpoint name."""
        return self.variables.values
