"""Horovod-shaped collective shim: RCCL over xGMI through the C ABI, torch.distributed for the rendezvous.

The reference drives data parallelism through ``horovod.torch`` (reference
bin/train_ce.py:83-131, bin/train_chain.py:106-145, bin/train_se.py:95-134,
data/dataloader.py:45-46,83-84).  This module offers the same call surface --
``init, size, rank, local_rank, broadcast_parameters, broadcast_optimizer_state,
DistributedOptimizer`` -- with one process per GPU:

* the gradient all-reduce is ``pk2_allreduce_bucket`` of libpk2hip.so (include/pk2hip.h: ``ncclAllReduce`` of RCCL
  on a communicator created by ``pk2_comm_init``); torch.distributed only carries the 128-byte unique id (through
  its store) and the one-time parameter broadcast.  Without a GPU / with the gloo backend (CPU tests, several
  ranks on one GPU) the same calls fall back to ``torch.distributed.all_reduce``;
* two schedules for the 85 MB flat gradient buffer: ONE all-reduce on the compute stream when backward is done, or
  one all-reduce per bucket (output layer, then LSTM layer 2, 1, 0: the order backward produces them) on a side HIP
  stream, overlapping the rest of backward.  Which is faster depends on the node (on ROCm 7.2 a second active stream
  slows the graph-replayed step chains: one rank, 35.4 -> 39.9 ms per step), so with more than one rank the choice is
  MEASURED at start-up: the two schedules alternate for a few steps, each step's (zero_grad -> gradients exchanged)
  GPU time is normalised by the GPU time of the same minibatch's forward pass, the ranks pool their means and all
  switch to the cheaper schedule.  PK2_HVD_OVERLAP=0/1 pins the schedule;
* the 1/size factor is folded into the optimiser kernel (no extra pass over the gradients);
* ``step()`` makes the compute stream wait on the side stream, so clipping acts on the averaged
  gradient (the reference clips local, possibly mid-flight gradients: SURVEY.md Appendix B#15).

Launch with ``python -m torch.distributed.run --nproc-per-node N ...`` (RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* from the environment).  Without those variables everything degrades to a
single process (size() == 1) and no process group is created.
"""
import ctypes as C
import os
import sys

import torch
import torch.distributed as dist

_state = dict(initialized=False, rank=0, size=1, local_rank=0, group=False, comm=None)


def init(backend=None):
    if _state["initialized"]:
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # PK2_HVD_SINGLE_RANK_GROUP=1 (tests): create the process group and run every collective even with one
    # rank, so the RCCL + side-stream path can be exercised on a one-GPU box.
    forced = os.environ.get("PK2_HVD_SINGLE_RANK_GROUP") == "1" and "RANK" in os.environ
    if world > 1 or forced:
        if backend is None:    # PK2_HVD_BACKEND=gloo: tests that put several ranks on one GPU (RCCL refuses that)
            backend = os.environ.get("PK2_HVD_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        local = int(os.environ.get("LOCAL_RANK", os.environ.get("RANK", "0")))
        if torch.cuda.is_available():
            torch.cuda.set_device(local % torch.cuda.device_count())
            _ranks_share_a_device(_local_world_size(), torch.cuda.device_count())
        if not dist.is_initialized():
            dist.init_process_group(backend=backend, rank=int(os.environ["RANK"]), world_size=world)
        _state.update(rank=dist.get_rank(), size=dist.get_world_size(), local_rank=local, group=True)
        if backend == "nccl" and torch.cuda.is_available() and os.environ.get("PK2_HVD_COMM", "pk2") == "pk2":
            # every rank must end up on the same path: a rank whose communicator could not be created tells the others
            try:
                comm, err = _create_comm(), ""
            except Exception as e:      # e.g. librccl not found: gradients then go through torch.distributed
                comm, err = None, str(e)
            ok = torch.tensor([1 if comm is not None else 0], device="cuda")
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 1:
                # Round 6 (the grouped call of pk2_allreduce_guarded has never run on more than one rank): both
                # entries are exercised ONCE here, on a small buffer, and checked against the closed form -- a node on which
                # they fail or give a wrong sum falls back to torch.distributed on EVERY rank instead of failing in step 1.
                err = _self_test_comm(comm)
                ok = torch.tensor([1 if not err else 0], device="cuda")
                dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                if int(ok.item()) != 1 and not err:
                    err = "a peer's self-test failed"
            if int(ok.item()) == 1:
                _state["comm"] = comm
            else:
                if comm is not None:
                    from . import _lib
                    _lib.lib().pk2_comm_destroy(comm)
                if _state["rank"] == 0:
                    sys.stderr.write("[hvd] library communicator unavailable (%s): gradients go through torch.distributed\n" % err)
    _state["initialized"] = True


def _local_world_size():
    """Ranks of this node, from whichever launcher started the job: torchrun (LOCAL_WORLD_SIZE), Open MPI / horovodrun
    (OMPI_COMM_WORLD_LOCAL_SIZE), MPICH / Intel MPI (MPI_LOCALNRANKS), Slurm (SLURM_NTASKS_PER_NODE).  None when nothing
    says: a multi-node job started without these variables has WORLD_SIZE > device_count on every node, and guessing
    "ranks share a GPU" from that silently took a correct one-process-per-GPU deployment off the persistent kernels
    (ADVICE r4)."""
    for k in ("LOCAL_WORLD_SIZE", "OMPI_COMM_WORLD_LOCAL_SIZE", "MPI_LOCALNRANKS", "SLURM_NTASKS_PER_NODE"):
        v = os.environ.get(k, "")
        digits = v.split("(")[0]
        if digits.isdigit() and int(digits) > 0:
            return int(digits)
    return None


def _ranks_share_a_device(local_world, devices):
    """One process per GPU is the deployment.  When several ranks of a node are mapped onto ONE device
    (tests that run the N-rank protocol on a one-GPU box), their persistent kernels -- each wants 32 co-resident
    workgroups on every XCD -- hold parts of the chip against each other until their polls time out, and since round 4 a
    time-out stops training (include/pk2hip.h: guard of the persistent kernels).  Such a job is switched to the
    launch-per-step kernels, which need no co-residency; explicit settings of the caller win."""
    if local_world is None or devices <= 0 or local_world <= devices:
        return
    changed = [k for k, v in (("PK2_LSTM_SEQ", "0"), ("PK2_LSTM_BIG_PERSIST", "0"), ("PK2_DEN_PERSIST", "0"),
                              ("PK2_LAT_DECODER", "frames")) if os.environ.setdefault(k, v) == v]
    if changed and os.environ.get("RANK", "0") == "0":
        sys.stderr.write("[hvd] %d local ranks on %d device(s): ranks share a GPU, persistent kernels off (%s)\n"
                         % (local_world, devices, ", ".join(changed)))


def _self_test_comm(comm):
    """One pk2_allreduce_bucket and one pk2_allreduce_guarded on 4096 floats through the new communicator: '' if both
    return rank sums / the guard maximum as they must, else what went wrong.  Never raises (every rank must reach the
    vote that follows)."""
    try:
        from . import _lib
        L = _lib.lib()
        r, w = dist.get_rank(), dist.get_world_size()
        st = torch.cuda.current_stream()
        want = float(w * (w + 1) // 2)
        for guarded in (False, True):
            t = torch.full((4096,), float(r + 1), device="cuda")
            slot = torch.tensor([1.0 if r == w - 1 else 0.0], device="cuda")
            if guarded:
                rc = L.pk2_allreduce_guarded(comm, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(slot.data_ptr()), C.c_void_p(st.cuda_stream))
            else:
                rc = L.pk2_allreduce_bucket(comm, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(st.cuda_stream))
            if rc != 0:
                msg = L.pk2_last_error()
                return "status %d: %s" % (rc, msg.decode() if msg else "")
            torch.cuda.synchronize()
            if not bool((t == want).all()):
                return "%s all-reduce returned %r, expected %r" % ("guarded" if guarded else "bucket", float(t[0].item()), want)
            if guarded and float(slot.item()) != 1.0:
                return "guard slot maximum %r, expected 1.0" % float(slot.item())
        return ""
    except Exception as e:      # noqa: BLE001
        return repr(e)[:200]


def _create_comm():
    """The library's own RCCL communicator (pk2_comm_init); the unique id travels through torch.distributed's store."""
    from . import _lib
    L = _lib.lib()
    n = int(L.pk2_comm_unique_id_bytes())
    store = dist.distributed_c10d._get_default_store()
    if dist.get_rank() == 0:
        buf = C.create_string_buffer(n)
        try:
            _lib.check(L.pk2_comm_unique_id(buf))
        except Exception:
            # the other ranks are blocked in store.get: tell them, so that every rank falls back together
            store.set("pk2_comm_unique_id", b"FAILED")
            raise
        store.set("pk2_comm_unique_id", buf.raw)
        uid = buf.raw
    else:
        uid = bytes(store.get("pk2_comm_unique_id"))
        if uid == b"FAILED":
            raise RuntimeError("rank 0 could not create the RCCL unique id")
    h = C.c_void_p()
    _lib.check(L.pk2_comm_init(dist.get_rank(), dist.get_world_size(), uid, C.byref(h)))
    return h


def comm_ranks():
    """Ranks of the communicator the gradients travel on: pk2_comm_info of the RCCL communicator, else the size of the
    torch.distributed group (gloo / CPU tests), else 1."""
    if _state["comm"] is not None:
        from . import _lib
        r, w = C.c_int32(-1), C.c_int32(-1)
        _lib.check(_lib.lib().pk2_comm_info(_state["comm"], C.byref(r), C.byref(w), None, 0))
        return int(w.value)
    return size()


def comm_library():
    """Path of the RCCL library behind the communicator ('' when gradients go through torch.distributed)."""
    if _state["comm"] is None:
        return ""
    from . import _lib
    buf = C.create_string_buffer(256)
    _lib.check(_lib.lib().pk2_comm_info(_state["comm"], None, None, buf, 256))
    return buf.value.decode()


def _allreduce_sum(t, stream=None, guard_slot=None):
    """In-place sum of a contiguous f32 tensor over the ranks, enqueued on `stream` (default: the current stream).
    `guard_slot` (a one-float device tensor, current stream only): its max over the ranks travels with the same call
    (pk2_allreduce_guarded: one RCCL group) -- the collective guard of DistributedOptimizer."""
    if _state["comm"] is not None and t.is_cuda:
        from . import _lib
        st = stream if stream is not None else torch.cuda.current_stream(t.device)
        _fake_peer(t, st)
        if guard_slot is not None:
            _lib.check(_lib.lib().pk2_allreduce_guarded(_state["comm"], C.c_void_p(t.data_ptr()), t.numel(),
                                                        C.c_void_p(guard_slot.data_ptr()), C.c_void_p(st.cuda_stream)))
        else:
            _lib.check(_lib.lib().pk2_allreduce_bucket(_state["comm"], C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(st.cuda_stream)))
        return
    if stream is not None and t.is_cuda:
        with torch.cuda.stream(stream):
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
    elif t.numel():
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    if guard_slot is not None:
        dist.all_reduce(guard_slot, op=dist.ReduceOp.MAX)


_peer_zeros = {}


def _fake_peer(t, st):
    """PK2_HVD_FAKE_PEER="blocks,passes" (one-GPU boxes: DESIGN.md 6, profiles/r05_peer_coresidency.txt): in front of every all-reduce
    call, on its stream, a kernel that does to the chip what the all-reduce kernel of an 8-rank job would -- `blocks`
    workgroups streaming a reduce-copy over the bucket `passes` times -- so that the schedules can be priced, and the
    persistent kernels' time-outs provoked, without a second GPU.  The bucket keeps its values (it adds zeros)."""
    spec = os.environ.get("PK2_HVD_FAKE_PEER")
    if not spec or t.numel() == 0:
        return
    from . import _lib
    blocks, passes = (int(v) for v in spec.split(","))
    z = _peer_zeros.get(t.device)
    if z is None or z.numel() < t.numel():
        z = _peer_zeros[t.device] = torch.zeros(max(t.numel(), 22_000_000), dtype=torch.float32, device=t.device)
    _lib.check(_lib.lib().pk2_debug_peer_reduce(C.c_void_p(t.data_ptr()), C.c_void_p(z.data_ptr()), t.numel(), blocks, passes,
                                                C.c_void_p(st.cuda_stream)))


# Collective guard (DistributedOptimizer): the stamp of the last exchanged step per device is PROCESS state, like the verdict
# ring it indexes (csrc/persist_guard.hip) -- a second optimiser of the same process (tests; SE after CE) must not restart at
# stamp 1 and read the ring words an earlier optimiser left behind as its own verdicts.
_GUARD_STAMP = {}
_LIVE_OPTIMIZERS = []          # weak references: shutdown() flushes their last verdicts


def finish():
    """Collective flush of every live DistributedOptimizer (call on all ranks at the same point: epoch end, before a checkpoint
    is written, before shutdown): raises on every rank when a persistent kernel timed out in one of the last steps."""
    for ref in list(_LIVE_OPTIMIZERS):
        opt = ref()
        if opt is None:
            _LIVE_OPTIMIZERS.remove(ref)
        else:
            opt.finish()


def shutdown():
    if _state["initialized"] or _LIVE_OPTIMIZERS:
        finish()
    if _state["comm"] is not None:
        from . import _lib
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        _lib.lib().pk2_comm_destroy(_state["comm"])
    if dist.is_initialized():
        dist.destroy_process_group()
    _state.update(initialized=False, rank=0, size=1, local_rank=0, group=False, comm=None)


def size():
    return _state["size"]


def rank():
    return _state["rank"]


def local_rank():
    return _state["local_rank"]


def local_device():
    """Index of this rank's GPU: the local rank (modulo the GPU count, which only matters when a test puts several
    ranks on one GPU)."""
    return _state["local_rank"] % max(1, torch.cuda.device_count())


def _collective():
    """True when gradients have to be exchanged (more than one rank, or the forced single-rank group)."""
    return _state["group"]


def broadcast_parameters(params, root_rank=0):
    """params: a state_dict or an iterable of (name, tensor) (reference bin/train_ce.py:127)."""
    if not _collective():
        return
    items = params.items() if hasattr(params, "items") else params
    for _, t in sorted(items, key=lambda kv: kv[0]):
        if torch.is_tensor(t):
            dist.broadcast(t, src=root_rank)


def _bcast_device():
    """Where a small control tensor has to live for the process group's backend (RCCL moves device memory only)."""
    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")


def _bcast_inplace(t, root_rank):
    """Broadcast into `t` itself, whatever device the backend wants the payload on."""
    dev = _bcast_device()
    if t.device.type == dev.type:
        dist.broadcast(t, src=root_rank)
    else:
        tmp = t.to(dev)
        dist.broadcast(tmp, src=root_rank)
        t.copy_(tmp)


def broadcast_optimizer_state(optimizer, root_rank=0):
    """Makes every rank's optimiser state equal to root's (reference bin/train_ce.py:128, after -resume_from_model).

    Root first broadcasts a HEADER -- the hyper-parameters of its param_groups and, per state tensor, whether it exists (flat
    optimisers) / its key, shape and dtype (torch.optim) -- and every rank makes its own state match that header before the
    tensors travel, so all ranks issue the same collectives whatever they held before (only root read the checkpoint; a rank
    with amsgrad moments root lacks; root without any state).  ADVICE r3.

    * pykaldi2_amd.optim optimisers (also behind DistributedOptimizer): the LIVE flat buffers (exp_avg, exp_avg_sq,
      max_exp_avg_sq / the momentum buffer) are broadcast in place (state_dict() hands out per-parameter COPIES: ADVICE r2);
      tensors root keeps on another device than the model are MOVED there, not re-created; a state root does not have is
      dropped on every rank (the usual fresh start: state is created by the first step).
    * any torch.optim optimiser: the tensors of optimizer.state in place, python numbers with the header."""
    if not _collective():
        return
    opt = getattr(optimizer, "_opt", optimizer)
    hyper_keys = ("lr", "betas", "eps", "weight_decay", "amsgrad", "momentum", "dampening", "nesterov", "maximize")

    def hyper_of(o):
        out = []
        for grp in o.param_groups:
            h = {k: grp[k] for k in hyper_keys if k in grp}
            for k in ("betas", "eps", "amsgrad", "momentum"):              # the flat optimisers keep these as attributes
                if k not in h and hasattr(o, k):
                    v = getattr(o, k)
                    h[k] = tuple(v) if isinstance(v, (list, tuple)) else v
            out.append(h)
        return out

    def apply_hyper(o, hyper):
        for grp, h in zip(o.param_groups, hyper):
            for k, v in h.items():
                if k in grp:
                    grp[k] = v
                elif hasattr(o, k):
                    setattr(o, k, list(v) if isinstance(getattr(o, k), list) else v)

    if hasattr(opt, "model") and hasattr(opt.model, "flat_parameters"):
        p, _ = opt.model.flat_parameters()
        adam = hasattr(opt, "betas")
        names = ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"] if adam else ["momentum_buffer"]

        def live():
            if adam:
                return [None] * len(names) if opt.state is None else [opt.state.get(k) for k in names]
            return [opt.buf]
        box = [dict(step=int(opt.step_count), have=[t is not None for t in live()], hyper=hyper_of(opt))]
        dist.broadcast_object_list(box, src=root_rank)
        hdr = box[0]
        apply_hyper(opt, hdr["hyper"])
        opt.step_count = hdr["step"]
        if not any(hdr["have"]):             # root has no state: every rank starts from zero moments, like root will
            if adam:
                opt.state = None
            else:
                opt.buf = None
            return
        cur = live()
        new = []
        for t, have in zip(cur, hdr["have"]):
            if not have:
                new.append(None)             # (e.g. a rank that ran with amsgrad while root did not)
            elif t is None:
                new.append(torch.zeros_like(p))
            elif t.device != p.device:
                new.append(t.to(p.device))   # root's checkpointed moments on another device: moved, not zeroed
            else:
                new.append(t)
        if adam:
            opt.state = dict(zip(names, new))
            if hasattr(opt, "amsgrad"):
                opt.amsgrad = new[2] is not None
        else:
            opt.buf = new[0]
        for t in new:
            if t is not None:
                _bcast_inplace(t, root_rank)
        return
    state = getattr(opt, "state", None)
    if not isinstance(state, dict):
        return
    params = [q for grp in opt.param_groups for q in grp["params"]]
    mine = []
    for q in params:
        st = state.get(q) if isinstance(state.get(q), dict) else {}
        mine.append({str(k): (("t", tuple(v.shape), str(v.dtype).replace("torch.", "")) if torch.is_tensor(v) else ("v", v))
                     for k, v in st.items()})
    box = [dict(state=mine, hyper=hyper_of(opt))]
    dist.broadcast_object_list(box, src=root_rank)
    hdr = box[0]
    apply_hyper(opt, hdr["hyper"])
    for q, want in zip(params, hdr["state"]):
        if not want:
            state.pop(q, None)
            continue
        st = state.setdefault(q, {})
        for k in [k for k in st if str(k) not in want]:
            del st[k]
        for k in sorted(want):
            spec = want[k]
            if spec[0] == "v":
                st[k] = spec[1]
                continue
            _, shape, dtype = spec
            dt = getattr(torch, dtype)
            v = st.get(k)
            if not torch.is_tensor(v) or tuple(v.shape) != tuple(shape) or v.dtype != dt:
                # (torch keeps `step` on the CPU unless capturable; everything else lives with the parameter)
                st[k] = v = torch.zeros(shape, dtype=dt, device="cpu" if k == "step" else q.device)
            _bcast_inplace(v, root_rank)


def allreduce_(tensor, average=True):
    if _collective():
        _allreduce_sum(tensor) if tensor.dtype == torch.float32 and tensor.is_contiguous() else dist.all_reduce(tensor, op=dist.ReduceOp.SUM)
        if average:
            tensor.div_(size())
    return tensor


class DistributedOptimizer:
    """hvd.DistributedOptimizer(optimizer, named_parameters=...) (reference bin/train_ce.py:131).

    Two kinds of wrapped optimiser:
    * a pykaldi2_amd.optim optimiser over a model with flat buffers: one all-reduce of the flat gradient buffer, or
      bucketed, stream-overlapped all-reduces driven by the model's bucket hook (see the module docstring for how the
      schedule is chosen); averaging folded into the update kernel;
    * any torch.optim optimiser: gradients are all-reduced (averaged) per parameter inside step().
    """

    TRIAL_STEPS = 6      # per schedule, after 2 warm-up steps

    def __init__(self, optimizer, named_parameters=None):
        self._opt = optimizer
        self._named = list(named_parameters) if named_parameters is not None else None
        self._flat = hasattr(optimizer, "model") and hasattr(optimizer.model, "flat_parameters")
        self._side = None
        model = getattr(optimizer, "model", None)
        # the bucketed schedule needs a model that reports finished buckets during backward (LSTMAM does, TransformerAM
        # does not: its gradients are exchanged in one piece)
        self._can_overlap = self._flat and callable(getattr(model, "_bucket_ready", None))
        env = os.environ.get("PK2_HVD_OVERLAP", "auto")
        self._mode = "single"
        self._trial = None
        if self._flat and _collective():
            optimizer.grad_scale = 1.0 / size()
            if self._can_overlap:
                model._bucket_hook = self._on_bucket
                if env == "1":
                    self._mode = "overlap"
                elif env != "0" and size() > 1:
                    self._trial = dict(step=0, sums={"single": 0.0, "overlap": 0.0}, n={"single": 0, "overlap": 0},
                                       ev_prev=None, ev_zero=None)
        self._overlap = self._mode == "overlap"     # (kept for introspection by tests)
        self._done = []          # [lo, hi) ranges of the flat gradient already exchanged in this step
        self._reduced = False
        # Collective guard of the persistent kernels: a rank whose one-launch kernel timed out holds a NaN-poisoned
        # gradient, and the all-reduce hands that NaN to every peer -- whose own guards are down.  So each rank's guard word
        # rides with the gradients (a one-float slot, max over the ranks, same RCCL group as the last piece of the
        # gradient), and every rank raises its own guard from the combined word BEFORE its optimiser kernel runs.  The
        # ranks also have to STOP together (a rank that raises alone leaves its peers blocked in the next all-reduce):
        # the combined word of step s is published in host-mapped memory, and every rank's step s + 2 reads the verdict
        # of step s -- the same word everywhere -- and raises Pk2Error there; the local, unsynchronised check of the
        # wrapped optimiser is switched off.  (Two steps back: the host never waits for the device in a healthy job.)
        self._guard_slot = None
        self._guard_dev = None
        self._guard_first = 1          # first stamp this optimiser issues (verdicts of earlier stamps belong to someone else)
        if self._flat and _collective() and torch.cuda.is_available() and os.environ.get("PK2_HVD_GUARD", "1") != "0":
            dev = next(iter(optimizer.model.parameters())).device
            if dev.type == "cuda":
                self._guard_slot = torch.zeros(1, dtype=torch.float32, device=dev)
                self._guard_dev = dev.index if dev.index is not None else torch.cuda.current_device()
                self._guard_first = _GUARD_STAMP.get(self._guard_dev, 0) + 1
                optimizer.guard_check = False
                import weakref
                _LIVE_OPTIMIZERS.append(weakref.ref(self))
        # bench.py / diagnostics: with `timing = []` every step appends the (start, end) device events of its all-reduce
        # calls, in issue order, on whichever stream they ran (bench.py reads them after its timed region)
        self.timing = None
        self._step_events = []

    def __getattr__(self, name):
        return getattr(self._opt, name)

    # bucket finished on the compute stream -> all-reduce it on the side stream
    def _on_bucket(self, name, grad_slice):
        if self._mode != "overlap":
            return
        if grad_slice.is_cuda:
            if self._side is None:
                self._side = torch.cuda.Stream(device=grad_slice.device)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(grad_slice.device))
            self._side.wait_event(ev)
            self._timed_allreduce(grad_slice, self._side)
        else:
            _allreduce_sum(grad_slice)
        lo, hi = self._opt.model._buckets[name]
        self._done.append((lo, hi))

    def synchronize(self):
        if self._flat and _collective() and not self._reduced:
            gflat = self._opt.model.flat_parameters()[1]        # the flat gradient buffer
            if self._side is not None:
                torch.cuda.current_stream().wait_stream(self._side)
            # whatever no bucket hook has covered (everything, in the single schedule; nothing, normally, in the
            # bucketed one; the whole buffer for a model without hooks) goes out now on the compute stream
            pos, pieces = 0, []
            for lo, hi in sorted(self._done) + [(gflat.numel(), gflat.numel())]:
                if lo > pos:
                    pieces.append((pos, lo))
                pos = max(pos, hi)
            slot = self._guard_slot if gflat.is_cuda else None
            if slot is not None:
                from . import _lib
                _lib.check(_lib.lib().pk2_persist_guard_export(_lib.ptr(slot), _lib.stream_ptr(slot.device)))
                if not pieces:
                    pieces = [(0, 0)]          # every bucket went out on the side stream: the slot travels alone
            for i, (lo, hi) in enumerate(pieces):
                self._timed_allreduce(gflat[lo:hi], None, slot if i == len(pieces) - 1 else None)
            if slot is not None:
                _GUARD_STAMP[self._guard_dev] = self._guard_stamp + 1
                _lib.check(_lib.lib().pk2_persist_guard_import(_lib.ptr(slot), self._guard_stamp, _lib.stream_ptr(slot.device)))
            self._done = []
            self._reduced = True
            self._trial_mark_exchanged()

    @property
    def _guard_stamp(self):
        return _GUARD_STAMP.get(self._guard_dev, 0)

    def finish(self):
        """Collective flush: the per-step check looks two steps back, so a time-out in the last two steps of a run
        or epoch would otherwise never be raised -- the job would exit 0 and write its checkpoint although those updates
        were skipped.  Waits for the device, then reads the verdicts of the last two exchanged steps; every rank sees the
        same combined words and raises (or not) together.  Called by the bin/train_*.py loops at epoch end and by
        hvd.shutdown()."""
        if self._guard_slot is None:
            return
        torch.cuda.synchronize(self._guard_slot.device)
        for back in (1, 0):
            self._guard_verdict(back)

    def _guard_verdict(self, back=2):
        """Raises on EVERY rank at the same step: the combined guard word of two steps ago (host-mapped, no device
        synchronisation in a healthy job: the device is never two whole steps behind the host for long)."""
        want = self._guard_stamp - back
        if self._guard_slot is None or want < self._guard_first:
            return
        import time
        from . import _lib
        ready, raised = C.c_uint32(0), C.c_uint32(0)
        t0 = None
        while True:
            _lib.check(_lib.lib().pk2_persist_guard_verdict(want, C.byref(ready), C.byref(raised)))
            if ready.value:
                break
            t0 = t0 or time.time()
            if time.time() - t0 > 120.0:
                raise _lib.Pk2Error("hvd: the guard verdict of step %d never arrived (device hung?)" % want)
            time.sleep(0.0002)
        _lib.check_persist_guard("DistributedOptimizer.step (rank %d, verdict of step %d over all ranks)" % (rank(), want),
                                 raised=bool(raised.value))

    def _timed_allreduce(self, t, stream, guard_slot=None):
        if self.timing is None or not t.is_cuda or t.numel() == 0:
            return _allreduce_sum(t, stream, guard_slot)
        st = stream if stream is not None else torch.cuda.current_stream(t.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        _allreduce_sum(t, stream, guard_slot)
        e1.record(st)
        self._step_events.append((e0, e1, int(t.numel()) * 4))

    def zero_grad(self, *a, **k):
        self._reduced = False
        self._done = []
        if self._trial is not None and torch.cuda.is_available():
            self._trial["ev_zero"] = torch.cuda.Event(enable_timing=True)
            self._trial["ev_zero"].record()
        return self._opt.zero_grad(*a, **k)

    def measure_grad_norm(self, max_norm):
        self.synchronize()  # the norm is taken over the summed gradient
        return self._opt.measure_grad_norm(max_norm)

    # ---- start-up trial: which schedule is cheaper on this node? --------------------------------------------------
    def _trial_mark_exchanged(self):
        tr = self._trial
        if tr is None or not torch.cuda.is_available():
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        tr["ev_sync"] = ev

    def _trial_step_done(self):
        tr = self._trial
        if tr is None:
            return
        if not torch.cuda.is_available():
            self._trial = None
            return
        ev_end = torch.cuda.Event(enable_timing=True)
        ev_end.record()
        if tr["step"] >= 2 and tr.get("ev_prev") is not None and tr.get("ev_zero") is not None and tr.get("ev_sync") is not None:
            tr["ev_sync"].synchronize()
            fwd = tr["ev_prev"].elapsed_time(tr["ev_zero"])       # forward pass + loss of this minibatch
            bwd = tr["ev_zero"].elapsed_time(tr["ev_sync"])       # backward until the gradients are exchanged
            if fwd > 0:
                tr["sums"][self._mode] += bwd / fwd
                tr["n"][self._mode] += 1
        tr["ev_prev"], tr["ev_zero"], tr["ev_sync"] = ev_end, None, None
        tr["step"] += 1
        if tr["step"] >= 2:
            self._mode = "overlap" if (tr["step"] - 2) % 2 else "single"
        if tr["step"] >= 2 + 2 * self.TRIAL_STEPS:
            means = torch.tensor([tr["sums"]["single"] / max(1, tr["n"]["single"]),
                                  tr["sums"]["overlap"] / max(1, tr["n"]["overlap"])], dtype=torch.float64,
                                 device="cuda" if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(means, op=dist.ReduceOp.SUM)           # every rank takes the same decision
            self._mode = "overlap" if float(means[1]) < float(means[0]) else "single"
            if rank() == 0:
                sys.stderr.write("[hvd] gradient exchange schedule: %s (backward+exchange / forward GPU time, mean over ranks: "
                                 "single %.3f, bucketed on a side stream %.3f)\n"
                                 % (self._mode, float(means[0]) / size(), float(means[1]) / size()))
            self._trial = None
        self._overlap = self._mode == "overlap"

    def step(self, *a, **k):
        if _collective():
            if self._flat:
                self.synchronize()
            else:
                params = [p for g in self._opt.param_groups for p in g["params"] if p.grad is not None]
                for p in params:
                    dist.all_reduce(p.grad, op=dist.ReduceOp.SUM)
                    p.grad.div_(size())
            self._guard_verdict()
        out = self._opt.step(*a, **k)
        # the exchange guard never depends on the caller invoking zero_grad(): gradients are overwritten by the next
        # backward, which must be followed by a fresh exchange
        self._reduced = False
        self._done = []
        if self.timing is not None:
            self.timing.append(self._step_events)
            self._step_events = []
        self._trial_step_done()
        return out
