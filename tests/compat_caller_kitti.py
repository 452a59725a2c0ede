"""A caller written against the reference's PUBLIC inference API only -- the same calls, in the same order, as the reference's
test_kitti.py makes (Config.load of the last results_kitti/Log_* folder, KITTIDataset(1, dl, load_test=True),
init_test_input_pipeline, KernelPointFCNN, ModelTester(model, restore_snap), tester.test_kitti) -- used by tests/test_gpu_kitti.py
on machines where the reference checkout itself is not present.  Run through `python -m d3feat_amd.compat_run`; reads data/kitti/
and results_kitti/Log_*/ from the working directory.  It calls test_kitti TWICE: the second call finds the per-pair files of the
first.  What each call returned goes to kitti_caller_<k>.npz for the test to compare."""
import os

import numpy as np

from datasets.KITTI import KITTIDataset
from models.KPFCNN_model import KernelPointFCNN
from utils.config import Config
from utils.tester import ModelTester

if __name__ == '__main__':
    logs = np.sort([os.path.join('results_kitti', f) for f in os.listdir('results_kitti') if f.startswith('Log')])
    path = logs[-1]
    config = Config()
    config.load(path)
    assert config.dataset.startswith('KITTI')
    dataset = KITTIDataset(1, config.first_subsampling_dl, load_test=True)
    dataset.init_test_input_pipeline(config)
    model = KernelPointFCNN(dataset.flat_inputs, config)
    snap_path = os.path.join(path, 'snapshots')
    snap_steps = [int(f[:-5].split('-')[-1]) for f in os.listdir(snap_path) if f[-5:] == '.meta']
    chosen_snap = os.path.join(path, 'snapshots', 'snap-{:d}'.format(np.sort(snap_steps)[-1]))
    tester = ModelTester(model, restore_snap=chosen_snap)
    for k in (1, 2):
        print("---- call %d ----" % k)
        out = tester.test_kitti(model, dataset)
        h = out.errors.host()
        np.savez("kitti_caller_%d.npz" % k, kp=out.kp.cpu().numpy(), count=out.count.cpu().numpy(), gt=out.gt.cpu().numpy(),
                 T=out.T.cpu().numpy(), rte=h["rte"], rre_deg=h["rre_deg"], flags=h["flags"], sums=h["sums"],
                 voxel_size=np.float64(dataset.voxel_size), experiment=np.array(tester.experiment_str))
