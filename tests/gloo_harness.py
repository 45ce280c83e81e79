"""
TEST-ONLY helper for the CPU gloo tests of csr_amd.dist: spawn(worker, world, *args) runs worker(rank, world, *args) in
`world` processes that share one gloo process group on a free local port.  `worker` must be a module-level function
(the processes are spawned, so it is pickled by name).
"""
import os
import socket
import sys

import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, worker, world, port, args):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        worker(rank, world, *args)
    finally:
        dist.destroy_process_group()


def spawn(worker, world, *args):
    mp.spawn(_rank, args=(worker, world, _free_port(), args), nprocs=world, join=True)
