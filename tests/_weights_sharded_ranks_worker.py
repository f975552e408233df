"""Worker of tests/test_dot_weights_sharded_gpu.py, one PROCESS per rank (torch.distributed.run): checks a-c of
tests/_weights_sharded_worker.py on one halo layout with a transport that crosses processes.
NKA_WS_MODE:
  p2p    every rank on cuda:0, the mailboxes mapped through hipIpc (nka_amd.dist.attach_allreduce, ladder = p2p only);
  rccl   one GPU per rank, the library's own RCCL communicator (ladder = rccl only).
Every rank drives two weighted handles on its slice -- ghosts that copy their owners, and ghosts of 1e3 * randn drawn fresh
every call -- and holds, after every call: decisions = the plain oracle's on the global vector, one digest and one red[] over
the ranks, the assembled owned entries within the truth rule at 1e-12, every ghost output equal to its owner's bits, and the
garbage twin's red[], h, c, digest, decisions and owned bits equal to the consistent one's."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nka_amd  # noqa: E402
from nka_amd import dist as nd  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
import overlap_layout as OL  # noqa: E402
import parity_util as P  # noqa: E402
from _sharded_ngpu_worker import small_inputs  # noqa: E402


def gathered(obj, world):
    out = [None] * world
    dist.all_gather_object(out, obj)
    return out


def main():
    mode = os.environ.get("NKA_WS_MODE", "p2p")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    local = int(os.environ.get("LOCAL_RANK", "0")) if mode == "rccl" else 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    n, halo = 240_011, 3
    ranks = OL.build(n, world, {"halo": halo})
    me = ranks[rank]
    own = torch.from_numpy(me.w != 0).to(dev)
    gen = torch.Generator(device=dev).manual_seed(50 + rank)
    for m, flavor, sums in ((5, 2, nka_amd.SUMS_AUTO), (20, 1, nka_amd.SUMS_BLOCKED)):
        tag = f"weights sharded over processes x{world} ({mode}, sums {sums}) n={n} m={m} flavor {flavor}"
        accs = []
        for how in ("device", "host"):
            a = nka_amd.nka().init(me.src.size, m, flavor=flavor, device=local).set_sum_order(sums)
            a.set_dot_weights(torch.from_numpy(me.w).to(dev) if how == "device" else me.w)
            hook = nd.attach_allreduce(a, rank, world, prefer=mode, ladder=(mode,))
            assert hook == mode and a.dot_weighted(), (hook, mode)
            accs.append(a)
        a, b = accs
        ora, spread = O.OracleNKA(n, m, flavor), P.Spread(O, n, m)
        for t, x in enumerate(small_inputs(n, m + 8, seed=77)):
            f = x.copy()
            ora.accel_update(f)
            spread.update(x)
            loc = torch.from_numpy(x[me.src]).to(dev)
            fa = loc.clone()
            a.accel_update(fa)
            fb = torch.where(own, loc, 1e3 * torch.randn(loc.numel(), generator=gen, dtype=torch.float64, device=dev))
            b.accel_update(fb)
            torch.cuda.synchronize()
            so, sa, sb = ora.state(), a.state(), b.state()
            # a. decisions and replication
            want = (ora.num_vec(), so.list_order(), so.free_order())
            for h, st in ((a, sa), (b, sb)):
                assert (h.num_vec(), st.list_order(), st.free_order()) == want, (tag, rank, t)
                digs = nd.replica_digests(h)
                assert all(d == digs[0] for d in digs), (tag, rank, t, [f"{d:016x}" for d in digs])
            reds = gathered(a.reductions(), world)
            assert all(np.array_equal(r, reds[0]) for r in reds), (tag, rank, t, "red[] differs between ranks")
            # b. the truth rule on the assembled owned entries
            got = OL.gather(ranks, gathered(fa.cpu().numpy(), world), n)
            err = float(np.linalg.norm(got - f) / np.linalg.norm(x))
            P.check(err, so, tag, base=1e-12, where=t, spread=spread.value, truth=spread.truth(got, x))
            # c. ghosts: the owner's output bits; garbage at the ghosts changes nothing that counts
            assert np.array_equal(fa.cpu().numpy(), got[me.src]), (tag, rank, t, "ghost outputs differ from their owners'")
            assert torch.equal(fa[own], fb[own]), (tag, rank, t, "garbage at the ghosts reached an owned entry")
            assert np.array_equal(a.reductions(), b.reductions()) and a.state_digest() == b.state_digest(), (tag, rank, t)
            assert np.array_equal(sa.h, sb.h) and np.array_equal(sa.c, sb.c), (tag, rank, t)
        P.finish()
        for slot in ora.state().list_order():
            for get in ("w", "v"):
                mine = getattr(a, get)(slot)
                assert np.array_equal(mine, OL.gather(ranks, gathered(mine, world), n)[me.src]), (tag, rank, "stored", get, slot)
                assert np.array_equal(getattr(b, get)(slot)[me.w != 0], mine[me.w != 0]), (tag, rank, "garbage twin: stored", get, slot)
        if rank == 0:
            rec = P.WORST[tag]
            print(f"{tag}: hook={hook} err_dev {rec['err_dev_exact']:.2e} err_ref {rec['err_ref_exact']:.2e}", flush=True)
        dist.barrier()                           # (nobody frees a mailbox a peer may still write into)
        a.delete()
        b.delete()
    print(f"rank {rank}/{world} weights over processes OK", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
