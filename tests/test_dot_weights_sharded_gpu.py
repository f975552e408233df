"""Diagonal dot-product weights (nka_hip_set_dot_weights) on SHARDED handles whose slices carry ghost / overlap entries:
w = 1 on the entries a slice owns, 0 on its ghosts, through every transport of the table of supported combinations
(include/nka_hip_ext.h) and both fast sum modes.

With such weights, and the owned entries of the slices in rank order being the global vector, the weighted sharded
accelerator is mathematically the plain accelerator on the deduplicated global vector
(tests/test_dot_weights_sharded_cpu.py holds that premise on the compiled reference), so the decisions are held to
oracle_py.OracleNKA(n_global), the values to the extended-precision trajectory under parity_util's truth rule, every reduced
sum to exact_sums.exact_dot -- and a ghost that held a copy of its owner's input holds its owner's OUTPUT bits afterwards.
The in-process checks a-g are listed in tests/_weights_sharded_worker.py, the layouts in tests/overlap_layout.py.

That the checks are not vacuous was shown once with mutated builds of the library (hook transport, never committed): the
weights ignored in ONE of k_dots / k_norm_diff / k_dots_win fail the truth rule b at the second call and, with the anchors
run alone, e (one more rank of ghosts); the norm exchange of the default sums skipped on a weighted handle fails a (red[]
differs between the ranks); a rank whose LOCAL sum d^2 is 0 taken for s == 0 fails a on the layout with a rank of ghosts
only (its decisions leave the other ranks')."""
import os
import subprocess
import sys

import numpy as np
import pytest

from launch_util import free_port, run_ranks
import overlap_layout as OL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_weights_sharded_worker.py")
RANKS_WORKER = os.path.join(ROOT, "tests", "_weights_sharded_ranks_worker.py")


@pytest.mark.parametrize("transport,sums", [("hook", "auto"), ("hook", "blocked"), ("p2p", "auto"), ("p2p", "blocked")])
def test_weighted_sharded_handles_with_ghost_entries(transport, sums):
    """One child process per (transport, sum mode): up to nine handles on their own streams and host threads (one hardware
    queue per stream: GPU_MAX_HW_QUEUES), every layout of overlap_layout.NAMES once -- halos of 1, 3, 512 and 700, a rank
    that owns nothing (ghosts only) first / in the middle / last, an empty rank, slices of one element, within one tile and
    beyond the hand-over of k_norm_diff's ahead loop, trailing ghost tiles -- with checks a-d and f after every call, then the
    bit anchors e and the life cycle g.  `hook`: the in-process rank-ordered hook through set_dot_prod; `p2p`: the mailboxes
    attached in-process (default sums: the send-and-gather kernel twice; SUMS_BLOCKED: fused into the final sums).  With a
    caller's hook nka_hip_clone lets the hook travel with the copy (as the reference's dp does), so "the copy refuses to
    update until it has an all-reduce of its own" is asserted with the mailboxes, which do not travel.
    The worker prints one line per layout and one per pair; a pair that silently skipped a layout, the anchors or the life
    cycle fails here."""
    env = dict(os.environ, OMP_NUM_THREADS="1", GPU_MAX_HW_QUEUES="16", NKA_WS_TRANSPORT=transport, NKA_WS_SUMS=sums)
    env.pop("NKA_WS_ONLY", None)
    p = subprocess.run([sys.executable, WORKER], env=env, capture_output=True, text=True, timeout=900)
    print(p.stdout[-6000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-6000:]
    pair = [ln for ln in p.stdout.splitlines() if ln.startswith("WEIGHTS SHARDED PAIR ")]
    assert len(pair) == 1 and pair[0].startswith(f"WEIGHTS SHARDED PAIR {transport} {sums}: "), p.stdout[-3000:]
    assert f"layouts {','.join(OL.NAMES)};" in pair[0] and "anchors and life cycle run" in pair[0], pair[0]
    per_layout = [ln for ln in p.stdout.splitlines() if ln.startswith("weights sharded ")]
    assert len(per_layout) == len(OL.NAMES) and all(f"({transport}, {sums})" in ln for ln in per_layout), p.stdout[-3000:]


def test_rccl_one_rank_with_general_weights():
    """h. The RCCL cell with the one rank this pool's boxes can form: general weights (not powers of two, 10 % zeros) on a
    handle with the library's own communicator give the bits of the same handle without a transport, in both sum modes."""
    import torch
    import nka_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    n, m = 100_003, 6
    rng = np.random.default_rng(12)
    w = np.exp2(rng.uniform(-3.0, 3.0, n))
    w[rng.random(n) < 0.1] = 0.0
    X = rng.standard_normal((m + 6, n))
    for order in (nka_amd.SUMS_AUTO, nka_amd.SUMS_BLOCKED):
        for flavor in (0, 1, 2):
            ref = nka_amd.nka().init(n, m, flavor=flavor).set_sum_order(order).set_dot_weights(w)
            acc = nka_amd.nka().init(n, m, flavor=flavor).set_sum_order(order).set_dot_weights(torch.from_numpy(w).cuda())
            acc.use_rccl(nka_amd.nka.rccl_unique_id(), 1, 0)
            assert acc.comm_info() == (1, 0) and acc.dot_weighted()
            for t in range(m + 6):
                fr, fa = torch.from_numpy(X[t].copy()).cuda(), torch.from_numpy(X[t].copy()).cuda()
                ref.accel_update(fr)
                acc.accel_update(fa)
                assert torch.equal(fr, fa), (order, flavor, t)
                np.testing.assert_array_equal(ref.reductions(), acc.reductions())
                assert ref.state_digest() == acc.state_digest(), (order, flavor, t)
            acc.drop_rccl()


def _run_ranks(world, mode, timeout):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", NKA_WS_MODE=mode)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), RANKS_WORKER]
    p = run_ranks(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-6000:]
    assert p.stdout.count("weights over processes OK") == world, p.stdout[-3000:]
    return p.stdout


def test_weighted_halo_layout_over_the_hipipc_mailboxes_between_processes():
    """i. Three processes sharing the GPU (five hold it: this test, the launcher, the ranks), their mailboxes mapped through
    hipIpc (nka_amd.dist.attach_allreduce, ladder = p2p only): checks a-c on a layout with halos of 3, default sums and
    SUMS_BLOCKED."""
    out = _run_ranks(3, "p2p", 600)
    assert out.count("hook=p2p") == 2, out[-2000:]


def test_weighted_halo_layout_over_rccl_n_gpus():
    """h, N ranks: the same over the library's own RCCL communicator, one GPU per rank.  Skips on a box with one GPU (RCCL
    refuses two ranks on one device): there the RCCL cell is held by the one-rank test above only."""
    import torch
    ngpu = min(torch.cuda.device_count(), 4)
    if ngpu < 2:
        pytest.skip("needs >= 2 GPUs (RCCL refuses two ranks on one device)")
    out = _run_ranks(ngpu, "rccl", 900)
    assert out.count("hook=rccl") == 2, out[-2000:]
