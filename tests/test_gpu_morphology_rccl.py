"""The tile-per-rank gather of Annotator.cell_morphology under RCCL ("nccl"): the feature rows are a HOST fp64 table, and RCCL moves device
buffers only, so dist.all_gather_rows stages a host tensor through the device as dist.all_reduce_sum does.  A process group of ONE rank on
cuda:0 with ``force_collective``, as tests/test_gpu_rccl_single_rank.py runs the device form: the same calls, dtypes and buffers a multi-rank
run makes (the two-rank layout runs under gloo in tests/test_gpu_morphology.py).  In a child process so that the group never leaks."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, os, sys
sys.path.insert(0, os.environ["RIBCA_ROOT"])
import numpy as np
import torch
import torch.distributed as tdist
from multiplexed_image_annotator_amd import dist, morphology
torch.cuda.set_device(0)
tdist.init_process_group("nccl", device_id=torch.device("cuda", 0))
width = 3 + len(morphology.FEATURES)
rows = np.random.RandomState(5).standard_normal((257, width))
rows[3, 7] = np.nan                                   # the circularity of a one-pixel cell
counts = np.zeros(1)
counts[0] = len(rows)
counts = dist.all_reduce_sum(torch.from_numpy(counts)).numpy()
send = torch.from_numpy(rows)
full = dist.all_gather_rows(send, len(rows), force_collective=True)
out = {"backend": tdist.get_backend(), "count": int(counts[0]), "host": not full.is_cuda, "dtype": str(full.dtype),
       "same_bytes": full.numpy().tobytes() == rows.tobytes(), "copied": full.data_ptr() != send.data_ptr()}
tdist.barrier()
tdist.destroy_process_group()
print(json.dumps(out))
"""


@pytest.mark.gpu
def test_a_host_table_is_gathered_through_the_device_under_rccl():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", RIBCA_ROOT=ROOT,
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out == {"backend": "nccl", "count": 257, "host": True, "dtype": "torch.float64", "same_bytes": True, "copied": True}
