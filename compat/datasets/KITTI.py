"""datasets.KITTI.KITTIDataset for the reference's unchanged test_kitti.py: the TEST split only (datasets/KITTI.py:62-80
constructor, :82-133 pair list, :135-243 generator, :245-256 mapping, :268-337 one pair).  Sweeps are read from
data/kitti/sequences/<drive>/velodyne/, poses from data/kitti/poses/, the ground truth of a pair from the cache
data/kitti/icp/<drive>_<t0>_<t1>.npy.  A pair without a cache file is an error unless the environment says
D3FEAT_KITTI_REFINE_GT=1 (refine_gt: the file is computed by the device ICP and written, as the reference does at :293-303 -- one
pair per device call, as the generator reads them; `python tools/kitti_icp.py --root data/kitti` fills the whole cache 16 pairs per
call and is the faster way, run it first), or
D3FEAT_KITTI_ODOMETRY_GT=1, which selects the unrefined odometry transform (:288-289) and writes nothing.
Training / validation splits and augmentation are out of scope."""
import os

import numpy as np
import open3d
import tensorflow as tf
import torch

from d3feat_amd.datasets import kitti
from datasets.common import Dataset


def make_open3d_point_cloud(xyz, color=None):
    pcd = open3d.geometry.PointCloud()
    pcd.points = open3d.utility.Vector3dVector(xyz)
    if color is not None:
        pcd.colors = open3d.utility.Vector3dVector(color)
    return pcd


def make_open3d_feature(data, dim, npts):
    feature = open3d.registration.Feature()
    feature.data = np.asarray(data).astype('d').transpose()
    return feature


class KITTIDataset(Dataset):
    DATA_FILES = {'test': 'data/kitti/config/test_kitti.txt'}

    def __init__(self, input_threads=8, first_subsampling_dl=0.30, load_test=False, refine_gt=None):
        Dataset.__init__(self, 'KITTI')
        self.network_model = 'descriptor'
        self.num_threads = input_threads
        self.load_test = load_test
        self.root = 'data/kitti/'
        self.icp_path = 'data/kitti/icp'
        self.voxel_size = first_subsampling_dl
        self.odometry_gt = os.environ.get("D3FEAT_KITTI_ODOMETRY_GT", "0") == "1"
        self.refine_gt = (os.environ.get("D3FEAT_KITTI_REFINE_GT", "0") == "1") if refine_gt is None else bool(refine_gt)
        self.anc_points = {'train': [], 'val': [], 'test': []}
        self.files = {'train': [], 'val': [], 'test': []}
        if not self.load_test:
            raise NotImplementedError("KITTIDataset(load_test=False): the training split is outside the inference path")
        self.prepare_kitti_ply('test')

    def prepare_kitti_ply(self, split='train'):
        """:82-126 (the sequences of config/test_kitti.txt when the file is there, 8 / 9 / 10 otherwise).  The sweeps are read
        pair by pair in the generator, not kept here."""
        if split != 'test':
            raise NotImplementedError("KITTIDataset: only the test split")
        seqs = kitti.TEST_SEQUENCES
        if os.path.exists(self.DATA_FILES[split]):
            seqs = [int(s) for s in open(self.DATA_FILES[split]).read().split()]
        self.files[split] = kitti.test_pairs(self.root, seqs)
        self.num_test = len(self.files[split])
        print("Num_test", self.num_test)

    def __getitem__(self, split, idx):
        """:268-337 for a test pair -> (aligned anchor, positive, anchor, positive, matches, trans, True)"""
        drive, t0, t1 = self.files[split][idx]
        trans = kitti.pair_transform(self.root, drive, t0, t1, icp_dir=self.icp_path, odometry_gt=self.odometry_gt,
                                     refine=self.refine_gt)
        xyz0, xyz1 = kitti.read_pair(self.root, drive, t0, t1)
        pcd0 = open3d.voxel_down_sample(make_open3d_point_cloud(xyz0), self.voxel_size)
        pcd1 = open3d.voxel_down_sample(make_open3d_point_cloud(xyz1), self.voxel_size)
        anc, pos = np.array(pcd0.points), np.array(pcd1.points)
        pcd0.transform(trans)
        return (np.array(pcd0.points), pos, anc, pos, np.array([]), trans, True)

    def get_batch_gen(self, split, config):
        if split != 'test':
            raise ValueError('Wrong split argument in data generator: ' + split)

        def gen():
            for p_i in range(self.num_test):
                aligned_anc, aligned_pos, anc, pos, _, trans, _ = self.__getitem__(split, p_i)
                drive, t0, t1 = self.files[split][p_i]
                anc_id, pos_id = str(drive) + "@" + str(t0), str(drive) + "@" + str(t1)
                yield (np.concatenate([anc, pos], axis=0), np.array([]), np.array([]), np.array([p_i, p_i], dtype=np.int32),
                       np.array([anc.shape[0], pos.shape[0]]), np.array([anc_id, pos_id]),
                       np.concatenate([aligned_anc, aligned_pos], axis=0), np.array(trans))
        gen_types = (tf.float32, tf.int32, tf.int32, tf.int32, tf.int32, tf.string, tf.float32, tf.float32)
        gen_shapes = ([None, 3], [None], [None], [None], [None], [None], [None, 3], [4, 4])
        return gen, gen_types, gen_shapes

    def _to_device(self, sample):
        trans = torch.from_numpy(np.ascontiguousarray(sample[7], dtype=np.float32)).to(self.device)
        return Dataset._to_device(self, sample[:7]) + (trans,)

    def get_tf_mapping(self, config):
        def tf_map(anc_points, anc_keypts, pos_keypts, obj_inds, stack_lengths, ply_id, backup_points, trans):
            batch_inds = self.tf_get_batch_inds(stack_lengths)
            stacked_features = tf.ones((tf.shape(anc_points)[0], 1), dtype=tf.float32)
            li = self.tf_descriptor_input(config, anc_points, stacked_features, stack_lengths, batch_inds)
            return li + [stack_lengths, anc_keypts, pos_keypts, ply_id, backup_points, trans]
        return tf_map
