"""KernelPointFCNN: the model class of the reference (models/KPFCNN_model.py:49-203), inference part.

    model = KernelPointFCNN(flat_inputs, config)          # same constructor signature
    model.anchor_inputs / out_features / out_scores / anc_id / pos_id / dropout_prob

`flat_inputs` is the positional list built by datasets/common.py:1410-1413 + the dataset tail
(datasets/ThreeDMatch.py:322; unpacked at KPFCNN_model.py:86-121), either as a list of tensors (the network is
evaluated immediately) or an iterator of such lists (dataset.flat_inputs; `run()` pulls the next element, which is
what one sess.run does in the reference).  Weights: a dict keyed by the checkpoint variable names (without the
`KernelPointNetwork/` root); missing variables are created like the reference's initialisers.

Of the loss graph (:143-191) the forward figures a validation fetches are here: after run() the attributes desc_loss, det_loss,
accuracy, ave_d_pos, ave_d_neg are device scalars (d3feat_amd/validation.py, one pair; safe_radius, keypts_num and det_loss_weight
from the config), the skip tuple (0, 0, -1, 0, 0) when flat_inputs carries no keypoint indices.  Gradients, the regularisation loss
and everything else of training are not part of this package.
"""
import numpy as np
import torch

from .. import validation
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
        """One forward pass = sess.run([out_features, out_scores], {dropout_prob: 1.0}) (utils/tester.py:198-199)."""
        if flat_inputs is None:
            flat_inputs = next(self.flat_inputs) if not isinstance(self.flat_inputs, (list, tuple)) else self.flat_inputs
        self.anchor_inputs = self.unpack(flat_inputs)
        with use_variables(self.variables):
            with self.variables.variable_scope('KernelPointNetwork'):
                pass
            self.out_features, self.out_scores = assemble_FCNN_blocks(self.anchor_inputs, self.config, self.dropout_prob)
        self._validation_figures()
        return self.out_features, self.out_scores

    def _validation_figures(self):
        """KPFCNN_model.py:131-186, forward: desc_loss (the circle loss), det_loss, accuracy, ave_d_pos, ave_d_neg of the pair just
        run, as device scalars."""
        anc, pos = self.anc_keypts_inds, self.pos_keypts_inds
        if isinstance(anc, np.ndarray) and isinstance(pos, np.ndarray) and anc.size > 0:     # as a dataset generator yields them
            anc = torch.from_numpy(np.ascontiguousarray(anc.reshape(-1), dtype=np.int32)).to(self.device)
            pos = torch.from_numpy(np.ascontiguousarray(pos.reshape(-1), dtype=np.int32)).to(self.device)
        # keypoint indices are DEVICE tensors (or what a generator yields, above); anything else in these two slots -- None, the empty
        # arrays of the test generators, a host placeholder -- is "no indices": the skip tuple, and no launch
        if not (isinstance(anc, torch.Tensor) and isinstance(pos, torch.Tensor) and anc.is_cuda and pos.is_cuda):
            if self._skip is None:
                self._skip = torch.tensor(validation.SKIP, dtype=torch.float32, device=self.device)
            self.validation = None
            self.desc_loss, self.det_loss, self.accuracy, self.ave_d_pos, self.ave_d_neg = self._skip.unbind(0)
            return
        cfg = self.config
        self.validation = validation.validation_pairs(
            self.out_features, self.out_scores, self.anchor_inputs['backup_points'], anc.reshape(-1).to(torch.int32),
            pos.reshape(-1).to(torch.int32), safe_radius=cfg.safe_radius, keypts_num=cfg.keypts_num,
            det_loss_weight=cfg.det_loss_weight)
        self.desc_loss, self.det_loss, self.accuracy, self.ave_d_pos, self.ave_d_neg = self.validation.figures(0)

    __call__ = run

    def weights(self):
        """All variables (numpy), keyed by checkpoint name."""
        return self.variables.values
