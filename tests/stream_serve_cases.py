"""Many video streams in one call (up_lstm_state_gather, up_lstm_serve_fwd; up_unipose_lstm_plan_pool_bytes,
up_unipose_lstm_serve_keypoints / _serve_frame_final_preds; ops.lstm_state_gather / lstm_serve_fwd; UniPoseLSTMPlan.stream_pool /
pool_view / serve / serve_frames; StreamSlots): shared by test_stream_serve_emu.py and test_stream_serve_gpu.py.

The yardstick is always an existing entry: up_lstm0_fwd / up_lstm_fwd on one sample's rows for the gate kernel, a numpy copy for the
gather, and for the plan programs the definition in include/unipose_hip.h — lane b of a serving call equals lane b of the plan's own
stream program at the same batch on the same input, "first" for a first or idle lane, "next" with that stream's state in lane b of
the state buffer (the other lanes zeros).  Every comparison is for equal bits; nothing here has a tolerance."""
import ctypes as C
import functools
import mmap

import numpy as np
import torch

from oracle import unipose_oracle as O
from unipose_amd import _C, ops, protocol

import lstm_plan_cases as lc
from protocol_cases import SENT, bits_equal, host

F32 = np.float32
SERVE = _C.PROGRAM_SERVE


def rup4(c):
    return (c + 3) // 4 * 4


def _st(t):
    return ops._stream(t)


def _i32(v):
    return (C.c_int32 * len(v))(*[int(i) for i in v])


def fenced(arr, front):
    """(emulator) a host tensor holding `arr` between two inaccessible pages, flush against the one in FRONT of it or against the one
    BEHIND it: an access one element outside on that side faults.  Each kernel case runs both ways."""
    import guard_alloc
    arr = np.ascontiguousarray(arr)
    page = mmap.PAGESIZE
    body = (max(arr.nbytes, 1) + page - 1) // page * page
    m = mmap.mmap(-1, 2 * page + body)
    addr = C.addressof(C.c_char.from_buffer(m))
    for guard in (addr, addr + page + body):
        if guard_alloc._libc.mprotect(C.c_void_p(guard), page, 0) != 0:
            raise OSError(C.get_errno(), "mprotect failed")
    guard_alloc._keep.append(m)
    off = page if front else page + body - arr.nbytes
    t = torch.from_numpy(np.frombuffer(m, dtype=arr.dtype, count=arr.size, offset=off).reshape(arr.shape))
    t.copy_(torch.from_numpy(arr))
    return t


def _put(dev, arr, fence=None):
    """`arr` on the device under test; fence: None, "front" or "back" (the emulator's guard pages)"""
    if fence is None:
        return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    return fenced(arr, fence == "front")


# ---- 1. the two kernels alone ------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [(cg, ldo, rps, B) for (cg, ldo) in ((15, 16), (17, 20)) for rps in (1, 20, 63, 64, 65) for B in (1, 3, 64)]


def tables(B, slots, kind, seed):
    """slot / first of B samples over `slots` > B records: the slots a permutation (lane b != slot b wherever the draw allows), and
    kind: "mixed" (first, continuing and, from B = 3 on, idle lanes), "first" (all first), "next" (all continuing), "idle" """
    rng = np.random.default_rng(seed)
    slot = rng.permutation(slots)[:B]
    if B > 1:
        assert (slot != np.arange(B)).any()
    first = np.zeros(B, np.int64)
    if kind == "first":
        first[:] = 1
    elif kind == "idle":
        slot[:] = -1
    elif kind == "mixed":
        first = (np.arange(B) + seed) % 2 if B > 1 else np.ones(1, np.int64)
        if B >= 3:
            first[0] = 0                                  # a continuing lane,
            slot[1] = -1                                  # an idle lane whose first flag is 0,
            first[1] = 0
            first[B - 1] = 1                              # a first lane; from B = 4 on an idle one whose flag is set
            slot[B - 1] = -1 if B > 3 else slot[B - 1]
    return [int(s) for s in slot], [int(f) for f in first]


def gate_inputs(cg, ldo, rps, B, slots, seed):
    """gates0 (rows, ldg0), gates (rows, ldg) with planted NaN / +-inf and large values, a pool of random BYTES whose cell rows
    (lanes < cg) hold numbers, some of them huge; row strides wider than the gates so that a stride slip shows"""
    rng = np.random.default_rng(seed)
    rows, ldg0, ldg = B * rps, rup4(3 * cg) + 4, rup4(4 * cg)
    g0 = (rng.standard_normal((rows, ldg0)) * 3).astype(F32)
    g1 = (rng.standard_normal((rows, ldg)) * 3).astype(F32)
    for g in (g0, g1):
        flat = g.reshape(-1)
        at = rng.choice(flat.size, size=min(8, flat.size), replace=False)
        flat[at] = np.resize(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 88.0, -104.0, 0.0], F32), at.size)
    stride = (2 * rps * ldo + 63) // 64 * 64
    pool = rng.integers(0, 256, (slots, stride * 4), dtype=np.uint8).view(F32).copy()
    cells = pool[:, rps * ldo:2 * rps * ldo].reshape(slots, rps, ldo).copy()
    cells[:, :, :cg] = (rng.standard_normal((slots, rps, cg)) * 2).astype(F32)
    big = rng.choice(slots * rps * cg, size=min(6, slots * rps * cg), replace=False)
    for n, v in zip(big, np.resize(np.array([1e30, -1e30, 3e38, -3e38, np.inf, np.nan], F32), big.size)):
        cells[n // (rps * cg), n // cg % rps, n % cg] = v
    pool[:, rps * ldo:2 * rps * ldo] = cells.reshape(slots, rps * ldo)
    return g0, g1, pool, stride


def serve_fwd_case(dev, cg, ldo, rps, B, fence=None):
    L = _C.lib()
    slots = B + 3
    rows = B * rps
    for kind in ("mixed", "first", "next", "idle"):
        seed = 1000 * cg + 10 * rps + B + len(kind)
        slot, first = tables(B, slots, kind, seed)
        g0, g1, pool0, stride = gate_inputs(cg, ldo, rps, B, slots, seed)
        if kind == "first":
            pool0 = np.full_like(pool0.view(np.uint8), 0xFF).view(F32)        # nothing of a fresh pool may reach an output
        tg0, tg1 = _put(dev, g0, fence), _put(dev, g1, fence)
        is_first = [s < 0 or f != 0 for s, f in zip(slot, first)]
        runs = []
        for _ in range(2):                                                      # twice from the same pool: equal bits
            pool = _put(dev, pool0, fence)
            cell = torch.full((rows, ldo), SENT).to(dev)
            hide = torch.full((rows, ldo), SENT).to(dev)
            _C.check(L.up_lstm_serve_fwd(tg0.data_ptr() if any(is_first) else None, g0.shape[1],
                                         tg1.data_ptr() if not all(is_first) else None, g1.shape[1], pool.data_ptr(), stride, slots,
                                         _i32(slot), _i32(first), cell.data_ptr(), hide.data_ptr(), ldo, B, rps, cg, _st(cell)),
                     "lstm_serve_fwd")
            runs.append((host(cell), host(hide), host(pool)))
        (cell, hide, pool), again = runs
        for a, b in zip(runs[0], again):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (kind, "two runs differ")
        assert (cell[:, cg:] == SENT).all() and (hide[:, cg:] == SENT).all()        # only lanes < Cg of cell / hide are written
        named = set()
        for b in range(B):
            r = slice(b * rps, (b + 1) * rps)
            rc = torch.full((rps, ldo), SENT).to(dev)
            rh = torch.full((rps, ldo), SENT).to(dev)
            if is_first[b]:
                tg = torch.from_numpy(g0[r].copy()).to(dev)
                _C.check(L.up_lstm0_fwd(tg.data_ptr(), g0.shape[1], rc.data_ptr(), rh.data_ptr(), ldo, rps, cg, _st(rc)), "lstm0_fwd")
            else:
                tg = torch.from_numpy(g1[r].copy()).to(dev)
                cp = torch.from_numpy(pool0[slot[b], rps * ldo:2 * rps * ldo].copy()).to(dev)
                _C.check(L.up_lstm_fwd(tg.data_ptr(), g1.shape[1], cp.data_ptr(), ldo, rc.data_ptr(), rh.data_ptr(), ldo, rps, cg,
                                       _st(rc)), "lstm_fwd")
            rc, rh = host(rc), host(rh)
            assert bits_equal(cell[r, :cg], rc[:, :cg]) and bits_equal(hide[r, :cg], rh[:, :cg]), (kind, b, slot[b], first[b])
            if kind == "first":
                assert np.isfinite(cell[r, :cg][np.isfinite(g0[r, :3 * cg]).all(1)]).all()
            if slot[b] < 0:
                continue
            named.add(slot[b])
            rec = pool[slot[b]]
            rec_h, rec_c = rec[:rps * ldo].reshape(rps, ldo), rec[rps * ldo:2 * rps * ldo].reshape(rps, ldo)
            assert bits_equal(rec_h[:, :cg], rh[:, :cg]) and bits_equal(rec_c[:, :cg], rc[:, :cg]), (kind, b, "record")
            assert (rec_h[:, cg:].view(np.int32) == 0).all() and (rec_c[:, cg:].view(np.int32) == 0).all()     # pad lanes: +0.0
            assert np.array_equal(rec[2 * rps * ldo:].view(np.int32), pool0[slot[b], 2 * rps * ldo:].view(np.int32))
        for s in range(slots):                                                  # records the table does not name keep every byte
            if s not in named:
                assert np.array_equal(pool[s].view(np.int32), pool0[s].view(np.int32)), (kind, s)
        if kind == "mixed" and B >= 3:
            assert any(is_first) and not all(is_first) and -1 in slot


def gather_case(dev, cg, ldo, rps, B, fence=None):
    L = _C.lib()
    slots = B + 3
    rows, ldd, coff = B * rps, ldo + 12, 8                                          # sentinel lanes left and right of coff
    for kind in ("mixed", "first", "next", "idle"):
        seed = 2000 * cg + 10 * rps + B + len(kind)
        slot, first = tables(B, slots, kind, seed)
        _, _, pool0, stride = gate_inputs(cg, ldo, rps, B, slots, seed)
        if kind in ("first", "idle"):
            pool0 = np.full_like(pool0.view(np.uint8), 0xFF).view(F32)
        pool = _put(dev, pool0, fence)
        dst = _put(dev, np.full((rows, ldd), SENT, F32), fence)
        _C.check(L.up_lstm_state_gather(pool.data_ptr(), stride, slots, _i32(slot), _i32(first), B, rps, ldo, dst.data_ptr(), ldd, coff,
                                        _st(dst)), "lstm_state_gather")
        got = host(dst)
        want = np.full((rows, ldd), SENT, F32)
        for b in range(B):
            cont = slot[b] >= 0 and not first[b]
            want[b * rps:(b + 1) * rps, coff:coff + ldo] = pool0[slot[b], :rps * ldo].reshape(rps, ldo) if cont else 0.0
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (kind, slot, first)
        assert np.array_equal(host(pool).view(np.int32), pool0.view(np.int32))              # the pool is only read


def kernel_refusal_case(dev):
    """each table error, B = 65, a NULL gate pointer that a sample needs: non-zero, outputs and pool untouched"""
    L = _C.lib()
    cg, ldo, rps, B, slots = 15, 16, 5, 3, 4
    g0, g1, pool0, stride = gate_inputs(cg, ldo, rps, B, slots, 5)
    tg0, tg1, pool = (torch.from_numpy(a.copy()).to(dev) for a in (g0, g1, pool0))
    cell = torch.full((B * rps, ldo), SENT).to(dev)
    hide = torch.full((B * rps, ldo), SENT).to(dev)
    dst = torch.full((B * rps, 2 * ldo), SENT).to(dev)
    many = list(range(65))
    ok = dict(g0=tg0.data_ptr(), ldg0=g0.shape[1], g=tg1.data_ptr(), ldg=g1.shape[1], pool=pool.data_ptr(), stride=stride, slots=slots,
              slot=[2, -1, 0], first=[1, 0, 0], cell=cell.data_ptr(), hide=hide.data_ptr(), ldo=ldo, B=B, rps=rps, cg=cg)

    def fwd(**kw):
        a = dict(ok, **kw)
        return L.up_lstm_serve_fwd(a["g0"], a["ldg0"], a["g"], a["ldg"], a["pool"], a["stride"], a["slots"],
                                   None if a["slot"] is None else _i32(a["slot"]), None if a["first"] is None else _i32(a["first"]),
                                   a["cell"], a["hide"], a["ldo"], a["B"], a["rps"], a["cg"], 0)

    def gather(**kw):
        a = dict(ok, **kw)
        return L.up_lstm_state_gather(a["pool"], a["stride"], a["slots"], None if a["slot"] is None else _i32(a["slot"]),
                                      None if a["first"] is None else _i32(a["first"]), a["B"], a["rps"], a["ldo"], dst.data_ptr(),
                                      a.get("ldd", 2 * ldo), a.get("coff", ldo), 0)
    bads = (dict(slot=[2, 4, 0]), dict(slot=[2, -2, 0]), dict(slot=[2, 0, 2]), dict(slot=[0, 1, 0], first=[1, 1, 1]), dict(B=0),
            dict(B=65, slots=80, slot=many, first=many), dict(slots=0), dict(slot=None), dict(first=None), dict(pool=None), dict(rps=0),
            dict(stride=2 * rps * ldo - 1), dict(ldo=0))
    for bad in bads:
        assert fwd(**bad) != 0, bad
        assert gather(**bad) != 0, bad
    for bad in (dict(g0=None), dict(g=None), dict(ldg0=3 * cg - 1), dict(ldg=4 * cg - 1), dict(cell=None), dict(hide=None), dict(cg=0),
                dict(ldo=cg - 1)):
        assert fwd(**bad) != 0, bad
    for bad in (dict(coff=-1), dict(coff=ldo + 1), dict(ldd=ldo, coff=1)):
        assert gather(**bad) != 0, bad
    assert (host(cell) == SENT).all() and (host(hide) == SENT).all() and (host(dst) == SENT).all()
    assert np.array_equal(host(pool).view(np.int32), pool0.view(np.int32))
    # a NULL gate pointer no sample needs is fine; -1 twice is fine (idle lanes share nothing)
    assert fwd(g=None, slot=[2, -1, -1], first=[1, 0, 0]) == 0
    assert fwd(g0=None, slot=[2, 1, 0], first=[0, 0, 0]) == 0
    assert gather() == 0 and fwd() == 0


def ops_case(dev):
    """ops.lstm_state_gather / ops.lstm_serve_fwd are the entries"""
    L = _C.lib()
    cg, ldo, rps, B, slots = 15, 16, 7, 3, 5
    g0, g1, pool0, stride = gate_inputs(cg, ldo, rps, B, slots, 11)
    slot, first = [3, -1, 0], [0, 0, 1]
    tg0, tg1 = torch.from_numpy(g0).to(dev), torch.from_numpy(g1).to(dev)
    res = []
    for through_ops in (True, False):
        pool = torch.from_numpy(pool0.copy()).to(dev)
        cell, hide = torch.full((B * rps, ldo), SENT).to(dev), torch.full((B * rps, ldo), SENT).to(dev)
        dst = torch.full((B, rps, 2 * ldo), SENT).to(dev)
        if through_ops:
            assert ops.lstm_state_gather(pool, slot, first, rps, ldo, dst, coff=ldo) is dst
            out = ops.lstm_serve_fwd(tg0, tg1, pool, slot, first, cell, hide, rps, cg)
            assert out[0] is cell and out[1] is hide
        else:
            _C.check(L.up_lstm_state_gather(pool.data_ptr(), stride, slots, _i32(slot), _i32(first), B, rps, ldo, dst.data_ptr(), 2 * ldo,
                                            ldo, _st(dst)), "lstm_state_gather")
            _C.check(L.up_lstm_serve_fwd(tg0.data_ptr(), g0.shape[1], tg1.data_ptr(), g1.shape[1], pool.data_ptr(), stride, slots,
                                         _i32(slot), _i32(first), cell.data_ptr(), hide.data_ptr(), ldo, B, rps, cg, _st(cell)),
                     "lstm_serve_fwd")
        res.append([host(t) for t in (dst, cell, hide, pool)])
    for a, b in zip(*res):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for bad in (lambda: ops.lstm_serve_fwd(tg0, tg1, pool, slot, first[:2], cell, hide, rps, cg),
                lambda: ops.lstm_serve_fwd(tg0, tg1, pool.view(-1), slot, first, cell, hide, rps, cg),
                lambda: ops.lstm_serve_fwd(tg0[:5], tg1, pool, slot, first, cell, hide, rps, cg),
                lambda: ops.lstm_state_gather(pool, slot, first, rps, ldo, dst[:2], coff=ldo)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("a bad call was not refused")


def stream_slots_case():
    from unipose_amd.plan import StreamSlots
    s = StreamSlots(3)
    got = [s.acquire() for _ in range(3)]
    assert got == [0, 1, 2] and s.free == 0
    try:
        s.acquire()
    except RuntimeError:
        pass
    else:
        raise AssertionError("exhaustion was not reported")
    s.release(1)
    assert s.free == 1
    for bad in (1, 3, -1):                                     # a double release, slots that never existed
        try:
            s.release(bad)
        except ValueError:
            continue
        raise AssertionError(f"release({bad}) was not refused")
    assert s.acquire() == 1
    s.release(2)
    s.release(0)
    assert s.acquire() == 0                                    # the lowest free slot first
    try:
        StreamSlots(0)
    except ValueError:
        pass
    else:
        raise AssertionError("StreamSlots(0) was not refused")


# ---- 2. the plan programs ----------------------------------------------------------------------------------------------------------------
FRAMES = 5
POOL_SLOTS = 6
# Streams, not lanes, have a history: S0 starts at frame 0; S1 is idle before frame 2 and starts there; S2 starts at frame 0, restarts at
# frame 3 and changes its slot there.  The lane a stream is served in is reversed between calls (lane order S0 S1 S2 on even frames,
# S2 S1 S0 on odd ones), and the slots are chosen so that no stream ever sits in the lane of its slot's number; 6 slots > B.  A plan of
# batch 2 serves S1 and S2 (S1's history holds S0's: a start, then continuing frames).
SLOT_OF = {"S0": [3, 3, 3, 3, 3], "S1": [-1, -1, 4, 4, 4], "S2": [1, 1, 1, 5, 5]}
SLOT_OF_B2 = {"S1": [-1, -1, 4, 4, 4], "S2": [3, 3, 3, 5, 5]}        # (S2 sits in lanes 1, 0, 1, 0, 1)
FIRST_OF = {"S0": [1, 0, 0, 0, 0], "S1": [0, 0, 1, 0, 0], "S2": [1, 0, 0, 1, 0]}


def schedule(B, j):
    """(streams in lane order, slot, first) of frame j"""
    names = ["S0", "S1", "S2"] if B == 3 else ["S1", "S2"]
    if j % 2:
        names = names[::-1]
    slot = [(SLOT_OF if B == 3 else SLOT_OF_B2)[n][j] for n in names]
    first = [FIRST_OF[n][j] for n in names]
    assert all(s != b for b, s in enumerate(slot))
    return names, slot, first


class ServeCtx:
    """One plan, its inputs, the figures it reported before any serving call, and the five calls of the schedule with the stream
    oracle of every lane — run once per configuration and shared, unchanged, by the tests."""

    def __init__(self, dev, K, B, H, W, output_stride, storage):
        from unipose_amd.plan import UniPoseLSTMPlan
        L = _C.lib()
        self.dev, self.K, self.B, self.H, self.W, self.storage = dev, K, B, H, W, storage
        if output_stride == 16:
            m = lc.lstm_model(dev, K)
        else:
            m = lc.mc.skeleton("lstm", K, output_stride=output_stride)
            m.load_state_dict(O.synth_state_dict(K, 4, lstm=True))
            m = m.to(dev).eval()
        self.model = m
        self.plan = plan = UniPoseLSTMPlan(m, B, H, W, storage=storage)
        self.figures = self.read_figures(plan)
        self.h, self.w, self.ldo = plan.out_height, plan.out_width, rup4(K + 2)
        self.x = O.synth_input((FRAMES, B, 3, H, W), 15).to(dev)
        self.cm = O.synth_input((FRAMES, B, 1, H, W), 16, "rand").to(dev)
        self.need = L.up_unipose_lstm_plan_program_workspace(plan._plan, SERVE)
        self.pool = plan.stream_pool(POOL_SLOTS)
        self.pool.fill_(0xFF)
        self.calls = []          # per frame: dict(slot, first, got=(preds, maxvals, idx, heat), before / after: the pool's bytes)
        self.lagged = plan.stream_pool(POOL_SLOTS)      # a second pool on the same plan, one frame behind, interleaved
        self.lagged.fill_(0xFF)
        self.lag_calls = []
        for j in range(FRAMES):
            self.calls.append(self.serve(self.pool, j, full=j == FRAMES - 1))
            if j >= 1:
                self.lag_calls.append(self.serve(self.lagged, j - 1))
        self.oracles = [self.oracle(j, self.calls[j], full=j == FRAMES - 1) for j in range(FRAMES)]

    @staticmethod
    def read_figures(plan):
        L = _C.lib()
        p = plan._plan
        return ([L.up_unipose_lstm_plan_workspace(p), L.up_unipose_lstm_plan_flip_workspace(p), L.up_unipose_lstm_plan_state_bytes(p)]
                + [L.up_unipose_lstm_plan_program_workspace(p, k) for k in list(range(10)) + [256 + k for k in range(10)]])

    def exact_ws(self, need):
        """a workspace of exactly `need` bytes, every byte 0xFF"""
        buf = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=self.dev)
        off = (-buf.data_ptr()) % 256
        return buf, buf.data_ptr() + off

    def serve(self, pool, j, full=False, plan=None):
        """frame j of the schedule through the C entry on `pool`, in a 0xFF workspace of exactly the reported size"""
        L = _C.lib()
        plan = plan or self.plan
        B, K, h, w = self.B, self.K, self.h, self.w
        _, slot, first = schedule(B, j)
        before = self.snapshot(pool)
        preds, mx = torch.full((B, K + 1, 2), SENT, device=self.dev), torch.full((B, K + 1, 1), SENT, device=self.dev)
        idx = torch.full((B, K + 1), -7, dtype=torch.int32, device=self.dev)
        heat = torch.full((B, K + 1, h, w), SENT, device=self.dev)
        keep, ws = self.exact_ws(self.need)
        oh, ow = (self.H, self.W) if full else (h, w)
        _C.check(L.up_unipose_lstm_serve_keypoints(plan._plan, self.x[j].data_ptr(), self.cm[j].data_ptr(), pool.data_ptr(), POOL_SLOTS,
                                                   _i32(slot), _i32(first), oh, ow, idx.data_ptr(), preds.data_ptr(), mx.data_ptr(),
                                                   heat.data_ptr(), ws, self.need, plan._stream()), "serve_keypoints")
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        del keep
        return dict(slot=slot, first=first, got=(preds, mx, idx, heat), before=before, after=self.snapshot(pool))

    def snapshot(self, pool):
        """the pool's bytes in a buffer that is a pool itself (aligned: pool_view takes it)"""
        copy = self.plan.stream_pool(POOL_SLOTS)
        copy.copy_(pool)
        return copy

    def state_views(self, state):
        """hide, cell (B, h, w, ldo) float32 views of a stream_state() buffer"""
        B, h, w, ldo = self.B, self.h, self.w, self.ldo
        v = state.view(torch.float32)
        half = v.numel() // 2
        return v[:half][:B * h * w * ldo].view(B, h, w, ldo), v[half:][:B * h * w * ldo].view(B, h, w, ldo)

    def oracle(self, j, call, full=False):
        """the plan's own stream program on the same full batch: first=True for the first and idle lanes; for the continuing lanes
        with a state buffer assembled from the pool's records before the call, the other lanes zeros.  Per lane: (preds, maxvals,
        idx, heat, new hide, new cell) — the last two None for an idle lane."""
        plan, B, K = self.plan, self.B, self.K
        recs = plan.pool_view(call["before"])
        lanes_first = [b for b in range(B) if call["slot"][b] < 0 or call["first"][b]]
        lanes_next = [b for b in range(B) if b not in lanes_first]
        out = [None] * B
        for lanes, is_first in ((lanes_first, True), (lanes_next, False)):
            if not lanes:
                continue
            state = plan.stream_state()
            hide, cell = self.state_views(state)
            if not is_first:
                for b in lanes:
                    hide[b] = recs[call["slot"][b], 0]
                    cell[b] = recs[call["slot"][b], 1]
            heat = torch.empty((B, K + 1, self.h, self.w), device=self.dev)
            preds, mx, idx = plan.stream(self.x[j], self.cm[j], state, first=is_first, full_resolution=full, heat=heat)
            for b in lanes:
                idle = call["slot"][b] < 0
                out[b] = (preds[b], mx[b], idx[b], heat[b], None if idle else hide[b].clone(), None if idle else cell[b].clone())
        return out


@functools.lru_cache(maxsize=None)
def ctx(dev, K=13, B=3, H=32, W=40, output_stride=16, storage="f32"):
    return ServeCtx(dev, K, B, H, W, output_stride, storage)


def _same(got, ref, what):
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert bits_equal(host(got), host(ref)), what


def _bytes_equal(a, b):
    return torch.equal(a.cpu(), b.cpu())


def schedule_case(c):
    """after every call: every lane's results and its record equal the stream oracle; records the table does not name, and all
    records for idle lanes, keep every byte"""
    plan = c.plan
    rec_bytes = c.pool.numel() // POOL_SLOTS
    seen = set()
    for j, (call, ora) in enumerate(zip(c.calls, c.oracles)):
        after = plan.pool_view(call["after"])
        for b in range(c.B):
            slot, first = call["slot"][b], call["first"][b]
            seen.add("idle" if slot < 0 else "first" if first else "next")
            for g, r, n in zip(call["got"], ora[b][:4], ("preds", "maxvals", "idx", "heat")):
                _same(g[b], r, (n, j, b))
            if slot >= 0:
                _same(after[slot, 0], ora[b][4], ("record hide", j, b))
                _same(after[slot, 1], ora[b][5], ("record cell", j, b))
                assert (host(after[slot])[..., c.K + 2:].view(np.int32) == 0).all()                 # pad lanes +0.0
        named = {s for s in call["slot"] if s >= 0}
        for s in range(POOL_SLOTS):
            if s not in named:
                r = slice(s * rec_bytes, (s + 1) * rec_bytes)
                assert _bytes_equal(call["after"][r], call["before"][r]), (j, s)
        if j:
            assert _bytes_equal(call["before"], c.calls[j - 1]["after"])
    assert seen == {"idle", "first", "next"}
    kinds = [{"f" if (s < 0 or f) else "n" for s, f in zip(call["slot"], call["first"])} for call in c.calls]
    assert {"f"} in kinds and {"n"} in kinds and {"f", "n"} in kinds          # both skipped-convolution paths and the full one ran
    # the restart: S2's first frame in a new slot equals a first frame, and its old record stays as it was
    assert SLOT_OF["S2"][2] != SLOT_OF["S2"][3]
    # the results depend on the state: a continuing lane differs from the same lane computed as a first frame
    j = FRAMES - 1
    st = plan.stream_state()
    fresh = plan.stream(c.x[j], c.cm[j], st, first=True, full_resolution=True)
    assert not bits_equal(host(fresh[1]), host(c.calls[j]["got"][1]))


def two_pools_case(c):
    """a second pool served one frame behind on the same plan, interleaved with the first: the same bits, one call later"""
    for j, call in enumerate(c.lag_calls):
        ref = c.calls[j]
        for g, r, n in zip(call["got"], ref["got"], ("preds", "maxvals", "idx", "heat")):
            _same(g, r, (n, j))
        assert _bytes_equal(call["after"], ref["after"]), j
    assert len(c.lag_calls) == FRAMES - 1


def idle_case(c):
    """an all-idle call through UniPoseLSTMPlan.serve leaves a 0xFF pool untouched and equals a first frame in every lane"""
    plan, B = c.plan, c.B
    pool = plan.stream_pool(2)
    pool.fill_(0xFF)
    heat = torch.full((B, c.K + 1, c.h, c.w), SENT, device=c.dev)
    got = plan.serve(c.x[0], c.cm[0], pool, [-1] * B, [0] * B, heat=heat)
    assert bool((pool == 0xFF).all())
    st = plan.stream_state()
    rh = torch.empty_like(heat)
    ref = plan.stream(c.x[0], c.cm[0], st, first=True, heat=rh)
    for g, r, n in zip(got + (heat,), ref + (rh,), ("preds", "maxvals", "idx", "heat")):
        _same(g, r, n)
    # pool_view: records of pool_bytes(1) bytes, hide then cell
    L = _C.lib()
    rec = L.up_unipose_lstm_plan_pool_bytes(plan._plan, 1)
    assert rec % 256 == 0 and 0 <= rec - 2 * c.h * c.w * c.ldo * 4 < 256 and L.up_unipose_lstm_plan_pool_bytes(plan._plan, 5) == 5 * rec
    assert L.up_unipose_lstm_plan_pool_bytes(plan._plan, 0) == 0 and L.up_unipose_lstm_plan_pool_bytes(None, 3) == 0
    v = plan.pool_view(pool)
    assert tuple(v.shape) == (2, 2, c.h, c.w, c.ldo) and v.dtype == torch.float32
    assert v.data_ptr() == pool.data_ptr() and v[1].data_ptr() == pool.data_ptr() + rec
    assert pool.data_ptr() % 256 == 0 and pool.dtype == torch.uint8 and pool.numel() == 2 * rec


def frames_case(c, frames=2):
    """serve_frames equals serve on the cropped frames and the centre maps, followed by ops.final_preds; the pools end equal"""
    plan, B, K, H, W, dev = c.plan, c.B, c.K, c.H, c.W, c.dev
    rng = np.random.default_rng(41)
    src = torch.from_numpy(rng.integers(0, 256, (3, 45, 60, 3), dtype=np.uint8)).to(dev)
    valid = [(45, 60), (40, 50), (45, 60)]
    pa, pb = plan.stream_pool(POOL_SLOTS), plan.stream_pool(POOL_SLOTS)
    pa.fill_(0xFF)
    pb.fill_(0xFF)
    for j in range(frames):
        # every stream starts in the first call; in the second all continue, served in the reversed lane order
        slot = [POOL_SLOTS - 1 - b for b in range(B)] if j % 2 == 0 else [POOL_SLOTS - B + b for b in range(B)]
        first = [1 if j == 0 else 0] * B
        cen = np.array([[28.0 + 4 * j + 2 * b, 20.0 + 2 * j - b] for b in range(B)])
        sc = np.array([0.2 + 0.02 * j + 0.03 * b for b in range(B)])
        cc = np.array([[W / 2 + j - b, H / 2 - 2 * j + b] for b in range(B)])
        fo = rng.integers(0, 3, (B,))
        heat = torch.full((B, K + 1, c.h, c.w), SENT, device=dev) if j == 0 else None
        got = plan.serve_frames(src, cen, sc, pa, slot, first, frame_of=fo, valid_hw=valid, crop_center=cc, heat=heat)
        assert len(got) == (3 if heat is None else 4)
        maps = protocol.crop_maps(cen, sc, [H, W], 0).reshape(B, 2, 3)
        x = ops.augment_image(src[torch.from_numpy(fo).to(dev)], maps, (H, W), valid_hw=np.asarray(valid)[fo])
        cm = ops.make_centermaps(cc, H, W, 3.0, device=dev)
        rheat = torch.empty((B, K + 1, c.h, c.w), device=dev)
        plan.serve(x, cm, pb, slot, first, heat=rheat)
        ref = ops.final_preds(rheat, cen, sc, return_coords=True)
        for g, r, n in zip(got, ref, ("preds", "coords", "maxvals")):
            _same(g, r, (n, j))
        if heat is not None:
            assert got[3] is heat
            _same(heat, rheat, ("heat", j))
        assert _bytes_equal(pa, pb), j
        assert not bits_equal(host(got[0]), host(got[1]))                              # the way back was taken


def figures_case(c):
    """no figure of the plan moved: as read before any serving call, and as a plan built afresh reports them"""
    L = _C.lib()
    p = c.plan._plan
    assert c.read_figures(c.plan) == c.figures
    assert all(f > 0 for f in c.figures[:3 + 9]) and c.figures[3 + 9] == 0
    assert L.up_unipose_lstm_plan_program_workspace(p, SERVE) > 0 and L.up_unipose_lstm_plan_program_workspace(p, SERVE + 1) > 0
    assert L.up_unipose_lstm_plan_program_workspace(p, SERVE + 2) == 0 and L.up_unipose_lstm_plan_program_workspace(p, SERVE - 1) == 0
    assert L.up_unipose_lstm_plan_program_workspace(None, SERVE) == 0
    assert L.up_abi_version() == 10


def one_pass_case(c, frames=2):
    """a plan created with UP_PLAN_FLIP_ONE_PASS serves the same bits"""
    from unipose_amd.plan import UniPoseLSTMPlan
    L = _C.lib()
    other = UniPoseLSTMPlan(c.model, c.B, c.H, c.W, storage=c.storage, flip="one_pass")
    assert L.up_unipose_lstm_plan_program_workspace(other._plan, SERVE) == c.need
    pool = other.stream_pool(POOL_SLOTS)
    pool.fill_(0xFF)
    for j in range(frames):
        call = c.serve(pool, j, plan=other)
        for g, r, n in zip(call["got"], c.calls[j]["got"], ("preds", "maxvals", "idx", "heat")):
            _same(g, r, (n, j))
        assert _bytes_equal(call["after"], c.calls[j]["after"]), j
    other.close()


def refusal_case(c):
    """every refusal of the serving entries, outputs and pool untouched"""
    L = _C.lib()
    plan, B, K, h, w, dev = c.plan, c.B, c.K, c.h, c.w, c.dev
    pool = plan.stream_pool(POOL_SLOTS)
    pool.fill_(0xFF)
    preds, mx = torch.full((B, K + 1, 2), SENT, device=dev), torch.full((B, K + 1, 1), SENT, device=dev)
    coords = torch.full((B, K + 1, 2), SENT, device=dev)
    heat = torch.full((B, K + 1, h, w), SENT, device=dev)
    need1 = L.up_unipose_lstm_plan_program_workspace(plan._plan, SERVE + 1)
    keep, ws = c.exact_ws(max(c.need, need1))
    _, slot, first = schedule(B, 0)
    ok = dict(x=c.x[0].data_ptr(), cm=c.cm[0].data_ptr(), pool=pool.data_ptr(), slots=POOL_SLOTS, slot=slot, first=first, oh=h, ow=w,
              preds=preds.data_ptr(), mx=mx.data_ptr(), ws=ws, nbytes=c.need)

    def keypoints(**kw):
        a = dict(ok, **kw)
        return L.up_unipose_lstm_serve_keypoints(plan._plan, a["x"], a["cm"], a["pool"], a["slots"],
                                                 None if a["slot"] is None else _i32(a["slot"]),
                                                 None if a["first"] is None else _i32(a["first"]), a["oh"], a["ow"], None, a["preds"],
                                                 a["mx"], heat.data_ptr(), a["ws"], a["nbytes"], 0)
    table_bads = (dict(slot=[POOL_SLOTS] + slot[1:]), dict(slot=[-2] + slot[1:]), dict(slot=[1] * B, first=[1] * B) if B > 1 else dict(slots=0),
                  dict(slots=0), dict(slots=1, slot=[1] + [-1] * (B - 1)), dict(slot=None), dict(first=None), dict(pool=None),
                  dict(pool=pool.data_ptr() + 64))
    other_bads = (dict(x=None), dict(cm=None), dict(preds=None), dict(mx=None), dict(ws=None), dict(ws=ws + 64), dict(oh=h + 1),
                  dict(nbytes=c.need - 256), dict(nbytes=0))
    for bad in table_bads + other_bads:
        assert keypoints(**bad) != 0, bad
    assert keypoints(nbytes=c.need - 256) == -4 and b"workspace" in L.up_last_error()
    # from frames
    src = torch.zeros((B, 20, 24, 3), dtype=torch.uint8, device=dev)
    args, keep2, _ = plan._frame_args("test", src, np.full((B, 2), 10.0), np.full((B,), 0.2), None, 0, None)
    cc = plan._crop_center("test", None, (B,))

    def frame(**kw):
        a = dict(ok, nbytes=need1, sigma=3.0, cc=cc.data_ptr(), res0=w, res1=h)
        a.update(kw)
        fa = list(args)
        if a.get("src") == "null":
            fa[0] = None
        return L.up_unipose_lstm_serve_frame_final_preds(plan._plan, *fa, a["cc"], a["sigma"], a["pool"], a["slots"],
                                                         None if a["slot"] is None else _i32(a["slot"]),
                                                         None if a["first"] is None else _i32(a["first"]), None, a["res0"], a["res1"],
                                                         a["preds"], coords.data_ptr(), a["mx"], heat.data_ptr(), a["ws"], a["nbytes"], 0)
    for bad in table_bads + (dict(src="null"), dict(cc=None), dict(sigma=0.0), dict(res0=0), dict(res1=-1), dict(preds=None), dict(mx=None),
                             dict(ws=None), dict(nbytes=need1 - 256)):
        assert frame(**bad) != 0, bad
    for t in (preds, mx, coords, heat):
        assert (host(t) == SENT).all()
    assert bool((pool == 0xFF).all())
    del keep, keep2
    # the Python methods: ValueError before any launch
    x, cm = c.x[0], c.cm[0]
    bad_calls = [
        lambda: plan.serve(x, cm, None, slot, first),
        lambda: plan.serve(x, cm, pool[:-1], slot, first),
        lambda: plan.serve(x, cm, pool.float(), slot, first),
        lambda: plan.serve(x, cm, pool, slot[:-1], first),
        lambda: plan.serve(x, cm, pool, slot, first + [0]),
        lambda: plan.serve(x[:, :, :8], cm, pool, slot, first),
        lambda: plan.serve(x, cm, pool, slot, first, heat=torch.empty(B, K + 1, h + 1, w, device=dev)),
        lambda: plan.pool_view(pool[:-4]),
        lambda: plan.stream_pool(0),
        lambda: plan.serve_frames(src, np.full((B, 2), 10.0), np.full((B,), 0.2), pool, slot[:-1], first),
        lambda: plan.serve_frames(src, np.full((B, 2), 10.0), np.full((B,), 0.2), pool, slot, first, res=[0, 4]),
    ]
    for i, call in enumerate(bad_calls):
        try:
            call()
        except ValueError:
            continue
        raise AssertionError(f"bad call {i} was not refused")
    # a table error reaches the caller as the library's error
    try:
        plan.serve(x, cm, pool, [0] * B if B > 1 else [POOL_SLOTS], [1] * B)
    except _C.UniPoseHipError:
        pass
    else:
        raise AssertionError("a bad table was not refused")
    assert bool((pool == 0xFF).all())


def big_batch_case(dev):
    """a plan of batch > UP_SERVE_CAP: UP_ERR_UNSUPPORTED from the serving entries only (no weights are needed to see it); unset
    weights are refused like the stream entries refuse them"""
    from unipose_amd.plan import _LstmConfig
    L = _C.lib()
    buf = torch.zeros(1 << 16).to(dev)
    p = buf.data_ptr() + (-buf.data_ptr()) % 256
    big = 1 << 40
    for batch, code, word in ((65, -2, b"batch"), (2, -1, b"never set")):
        plan = C.c_void_p()
        assert L.up_unipose_lstm_plan_create(C.byref(_LstmConfig(batch, 1, 32, 32, 16, 13)), C.byref(plan)) == 0
        slot, first = _i32([-1] * batch), _i32([0] * batch)
        assert L.up_unipose_lstm_plan_pool_bytes(plan, 3) == 3 * 2 * 4 * 4 * 16 * 4
        assert L.up_unipose_lstm_serve_keypoints(plan, p, p, p, 3, slot, first, 4, 4, None, p, p, None, p, big, 0) == code
        assert word in L.up_last_error()
        assert L.up_unipose_lstm_serve_frame_final_preds(plan, p, 0, batch, 8, 8, None, None, p, 128.0, 128.0, 256.0, p, 3.0, p, 3, slot,
                                                         first, None, 4, 4, p, None, p, None, p, big, 0) == code
        assert word in L.up_last_error()
        if batch == 65:          # ... and the stream entry of the same plan gets as far as the weights
            assert L.up_unipose_lstm_stream_keypoints(plan, p, p, p, 1, 4, 4, None, p, p, None, p, big, 0) == -1
            assert b"never set" in L.up_last_error()
        L.up_unipose_lstm_plan_destroy(plan)
    assert not buf.any()
