"""A caller written against the reference's PUBLIC inference API only -- the same calls, in the same order, as the reference's
test_eth.py makes (Config.load of the last results/Log_* folder whose dataset starts with ETH, the stop in pdb.set_trace(), the three
configuration edits, ETHDataset(1, load_test=True), init_test_input_pipeline, KernelPointFCNN, ModelTester(model, restore_snap),
tester.generate_descriptor) -- used by tests/test_gpu_eth.py on machines where the reference checkout itself is not present.  Run
through `python -m d3feat_amd.compat_run`; reads data/ETH/ and results/Log_*/ from the working directory."""
import os

import numpy as np

from datasets.ETH import ETHDataset
from models.KPFCNN_model import KernelPointFCNN
from utils.config import Config
from utils.tester import ModelTester

if __name__ == '__main__':
    logs = np.sort([os.path.join('results', f) for f in os.listdir('results') if f.startswith('Log')])
    path = None
    for log in logs[::-1]:
        log_config = Config()
        log_config.load(log)
        if log_config.dataset.startswith('ETH'):
            path = log
            break
    assert path is not None
    config = Config()
    config.load(path)
    import pdb
    pdb.set_trace()
    config.first_subsampling_dl = 0.05
    config.dataset = 'ETH'
    config.KP_extent = 2
    dataset = ETHDataset(1, load_test=True)
    dataset.init_test_input_pipeline(config)
    model = KernelPointFCNN(dataset.flat_inputs, config)
    snap_path = os.path.join(path, 'snapshots')
    snap_steps = [int(f[:-5].split('-')[-1]) for f in os.listdir(snap_path) if f[-5:] == '.meta']
    chosen_snap = os.path.join(path, 'snapshots', 'snap-{:d}'.format(np.sort(snap_steps)[-1]))
    tester = ModelTester(model, restore_snap=chosen_snap)
    tester.generate_descriptor(model, dataset)
    np.savez("eth_caller.npz", experiment=np.array(tester.experiment_str), limits=np.asarray(dataset.neighborhood_limits),
             ids=np.array(dataset.ids_list['test']))
