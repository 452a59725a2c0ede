"""utils.tester.ModelTester for the reference's unchanged test_3dmatch.py and test_kitti.py (utils/tester.py:136-360): same
constructor, same `generate_descriptor(model, dataset)` with its three files per fragment under
geometric_registration/D3Feat_<experiment>/{descriptors,keypoints,scores}/<scene>/, same `test_kitti(model, dataset)` with its
per-pair files under geometric_registration_kitti/D3Feat_<experiment>-pred250/ and its log lines -- the session / saver objects
come from the compat `tensorflow`, every forward pass is the HIP path."""
import logging
import os
import sys
import time

import numpy as np
import tensorflow as tf
import torch

from d3feat_amd import keypoints, registration
from d3feat_amd.utils import results
from d3feat_amd.utils.results import save_3dmatch_results


class ModelTester:
    def __init__(self, model, restore_snap=None):
        my_vars = tf.get_collection(tf.GraphKeys.GLOBAL_VARIABLES, scope='KernelPointNetwork')
        self.saver = tf.train.Saver(my_vars, max_to_keep=100)
        cProto = tf.ConfigProto(log_device_placement=False, allow_soft_placement=True)
        cProto.gpu_options.allow_growth = True
        self.sess = tf.Session(config=cProto)
        self.sess.run(tf.global_variables_initializer())
        self.experiment_str = 'init'
        if restore_snap is not None:
            self.saver.restore(self.sess, restore_snap)
            print("Model restored from " + restore_snap)
            # '<...>_<timestamp>/snapshots/snap-<step>' -> '<timestamp[:8]>-<step>' (utils/tester.py:163)
            self.experiment_str = restore_snap.split("_")[-1][:8] + "-" + restore_snap.split("-")[-1]

    def generate_descriptor(self, model, dataset):
        """One forward pass per test fragment (self-pair); keypoints / descriptors / scores of the first cloud, rows in
        ascending score order, as .npy files (utils/tester.py:166-231)."""
        self.sess.run(dataset.test_init_op)
        self.experiment_str = self.experiment_str + '-pred'
        root = 'geometric_registration/D3Feat_%s' % self.experiment_str
        t = []
        for _ in range(dataset.num_test):
            stime = time.time()
            inputs, features, scores, anc_id = self.sess.run(
                [model.anchor_inputs, model.out_features, model.out_scores, model.anc_id], {model.dropout_prob: 1.0})
            t.append(time.time() - stime)
            first_len = int(inputs['in_batches'][0].shape[0] - 1)      # the row holds one pad entry (equal lengths)
            save_3dmatch_results(root, anc_id, inputs['backup_points'], features, scores, first_len)
            name = anc_id.decode("utf-8")
            print("Generate cloud_bin_{0} for {1}".format(int(name.split("_")[-1][:-4]), name.split("/")[0]))
            print("*" * 40)
        print("Avergae Feature Extraction Time:", np.mean(t))

    def test_kitti(self, model, dataset):
        """utils/tester.py:235-360 without the per-pair round trip: one forward pass per test pair, the 250 best rows of each cloud
        picked on the device (keypoints.topk), then ALL pairs registered and scored in one registration.register_kitti_pairs call.
        An existing <anc>-<pos>.npz of a pair overrides its transform (:299-302), new ones are written (:317-323), the reference's
        log lines are printed (results.kitti_lines)."""
        self.sess.run(dataset.test_init_op)
        num_keypts = 250
        icp_save_path = f'geometric_registration_kitti/D3Feat_{self.experiment_str}-pred{num_keypts}'
        os.makedirs(icp_save_path, exist_ok=True)
        ch = logging.StreamHandler(sys.stdout)
        logging.getLogger().setLevel(logging.INFO)
        logging.basicConfig(format='%(asctime)s %(message)s', datefmt='%m/%d %H:%M:%S', handlers=[ch])

        blocks, counts, gts, ids, feat_times = [], [], [], [], []
        for _ in range(dataset.num_test):
            stime = time.time()
            anc_id, pos_id = self.sess.run([model.anc_id, model.pos_id], {model.dropout_prob: 1.0})
            inner = model.inner                                       # the device tensors of the pass just made
            a = inner.anchor_inputs
            kp, cnt = keypoints.topk(a['points'][0], inner.out_features, inner.out_scores, num_keypts, lens=a['stack_lengths'])
            torch.cuda.synchronize()
            feat_times.append(time.time() - stime)
            blocks.append(kp)
            counts.append(cnt)
            gts.append(a['trans'][:3])
            ids.append((anc_id, pos_id))
        P = len(ids)
        if P == 0:
            return None
        kp, count = torch.cat(blocks, 0).contiguous(), torch.cat(counts, 0).contiguous()
        gt = torch.stack(gts, 0).to(torch.float32).contiguous()
        stime = time.time()
        out = registration.register_kitti_pairs(kp, count, gt, dataset.voxel_size)
        # files of an earlier run override the transforms of their pairs
        paths = [os.path.join(icp_save_path, results.kitti_pair_filename(a, p)) for a, p in ids]
        have = [p for p in range(P) if os.path.exists(paths[p])]
        if have:
            T = out.T.cpu()
            for p in have:
                T[p] = torch.from_numpy(np.asarray(np.load(paths[p])['trans'], np.float32)[:3])
                print(f"Read from {paths[p]}")
            out.T.copy_(T)
            registration.pose_errors(out.T, gt, out=out.errors, **registration.KITTI_SUCCESS)
        h = out.errors.host()
        reg_time = (time.time() - stime) / P
        if len(have) < P:
            T, rec, n = out.T.cpu().numpy(), kp.cpu().numpy(), count.cpu().numpy()
            for p in (p for p in range(P) if p not in set(have)):
                s, t = rec[2 * p, :n[2 * p]], rec[2 * p + 1, :n[2 * p + 1]]
                results.save_kitti_pair(icp_save_path, ids[p][0], ids[p][1], T[p], s[:, :3], t[:, :3], s[:, -1:], t[:, -1:])
        for line in results.kitti_lines([a for a, _ in ids], h["rte"][:, 0], h["rre_deg"][:, 0], h["flags"][:, 0], feat_times=feat_times,
                                        reg_times=[reg_time] * P, final=out.errors.meters()):
            logging.info(line)
        out.kp, out.count, out.gt, out.ids = kp, count, gt, ids
        return out
