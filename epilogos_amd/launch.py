"""`epilogos --gpus N` from a plain start: how many GPUs there are to use, and one process per GPU under torch.distributed.run, started
as a child of a process that has neither imported torch nor touched a GPU (run.py reaches these through its own names)."""
import os
import sys
from pathlib import Path


def _visible_gpus():
    """GPUs this process could use, counted WITHOUT loading torch or touching HIP (the parent of the ranks must stay
    GPU-free): the KFD topology lists every compute node (a GPU has simd_count > 0, a CPU node 0), and the usual
    *_VISIBLE_DEVICES lists narrow it down."""
    n = 0
    try:
        for node in sorted(Path("/sys/class/kfd/kfd/topology/nodes").iterdir()):
            props = dict(l.split()[:2] for l in (node / "properties").read_text().splitlines() if len(l.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except (OSError, ValueError):
        n = 0
    # a container may see the host's whole KFD topology and only some of its render nodes: a GPU without an accessible
    # /dev/dri/renderD* cannot be opened (a rank on it would die in torch.cuda.set_device)
    try:
        usable = len([d for d in Path("/dev/dri").iterdir() if d.name.startswith("renderD") and os.access(d, os.R_OK | os.W_OK)])
        if n and usable:
            n = min(n, usable)
    except OSError:
        pass
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            listed = len([t for t in v.split(",") if t.strip()])
            n = min(n, listed) if n else listed
    return max(n, 1)


def _strip_gpus(argv):
    """The argument list without --gpus (the children learn their number from WORLD_SIZE)."""
    from .helpers import splitGpusOption
    return splitGpusOption(argv)[1]


def _launch_command(gpus, argv, port):
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
            "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "epilogos_amd.run"] + _strip_gpus(argv)


def _launch(gpus, argv):
    """One process per GPU under torch.distributed.run, as a child of this (GPU-free) process; its exit code is ours."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or gpus) // gpus)))
    root = str(Path(__file__).resolve().parents[1])
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    cmd = _launch_command(gpus, argv, port)
    if os.environ.get("EPILOGOS_LAUNCH_DRYRUN"):
        print(" ".join(cmd))
        return 0
    return subprocess.call(cmd, env=env)
