"""datasets.ETH.ETHDataset for the reference's unchanged test_eth.py (datasets/ETH.py:21-44 constructor, :46-136 generator, :138-150
mapping, :152-189 prepare_geometry_registration_eth).  Scans are read from data/ETH/<scene>/*.ply in the order of their trailing
number and voxelised at 0.0625 m (open3d.voxel_down_sample of the compat tree: this project's grid subsampler, not Open3D's voxel
grid); every scan is fed stacked with itself (anc == pos, :85-90).  There is no training split (the reference exits there)."""
import os
from os.path import join

import numpy as np
import open3d
import tensorflow as tf

from d3feat_amd.datasets.eth import SCENES, VOXEL_SIZE, scene_scans
from datasets.common import Dataset


class ETHDataset(Dataset):
    def __init__(self, input_threads=8, load_test=False):
        Dataset.__init__(self, 'ETH')
        self.network_model = 'descriptor'
        self.num_threads = input_threads
        self.load_test = load_test
        self.root = 'data/ETH'
        self.anc_points = {'test': []}
        self.ids_list = {'test': []}
        self.num_test = 0
        if not self.load_test:
            raise NotImplementedError("ETHDataset(load_test=False): the reference has no training split of ETH (it exits)")
        self.prepare_geometry_registration_eth()

    def prepare_geometry_registration_eth(self):
        """:152-189.  Scenes absent from data/ETH are skipped (the reference would stop at the first one); no scene at all is an
        error."""
        self.num_test = 0
        found = [s for s in SCENES if os.path.isdir(join(self.root, s))]
        if not found:
            raise FileNotFoundError("%s holds none of the ETH scenes %s" % (self.root, list(SCENES)))
        for scene in found:
            for path in scene_scans(self.root, scene):
                pcd = open3d.voxel_down_sample(open3d.read_point_cloud(path), voxel_size=VOXEL_SIZE)
                points = np.asarray(pcd.points)
                print(points.shape)
                self.anc_points['test'].append(points)
                self.ids_list['test'].append(scene + '/' + os.path.basename(path))
                self.num_test += 1

    def get_batch_gen(self, split, config):
        if split != 'test':
            raise ValueError('Wrong split argument in data generator: ' + split)

        def gen():
            print(np.arange(self.num_test))
            for i in range(self.num_test):
                pts = self.anc_points['test'][i].astype(np.float32)
                fid = self.ids_list['test'][i]
                stacked = np.concatenate([pts, pts], axis=0)
                yield (stacked, np.array([]), np.array([]), np.array([i, i], dtype=np.int32),
                       np.array([pts.shape[0], pts.shape[0]]), np.array([fid, fid]), stacked)
        gen_types = (tf.float32, tf.int32, tf.int32, tf.int32, tf.int32, tf.string, tf.float32)
        gen_shapes = ([None, 3], [None], [None], [None], [None], [None], [None, 3])
        return gen, gen_types, gen_shapes

    def get_tf_mapping(self, config):
        def tf_map(anc_points, anc_keypts, pos_keypts, obj_inds, stack_lengths, ply_id, backup_points):
            batch_inds = self.tf_get_batch_inds(stack_lengths)
            stacked_features = tf.ones((tf.shape(anc_points)[0], 1), dtype=tf.float32)
            li = self.tf_descriptor_input(config, anc_points, stacked_features, stack_lengths, batch_inds)
            return li + [stack_lengths, anc_keypts, pos_keypts, ply_id, backup_points]
        return tf_map
