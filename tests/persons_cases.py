"""Multi-person decode of a whole batch in one launch (up_persons_decode, up_unipose_persons; ops.persons_decode,
ops.persons_decode_nhwc, ops.uniPose_kpts_batch, UniPosePlan.persons): shared by the emulator and the GPU tests.

Every comparison is of exact integers.  The yardsticks are the G9 fixture (outputs and exception types of the reference's own
uniPose_kpts), the numpy restatement oracle.unipose_kpts_multi, and the project's earlier path ops.uniPose_kpts (up_peak_mask,
host lists, up_box_argmax), which the new kernel does not go through."""
import ctypes as C
import os

import numpy as np
import torch

from oracle import unipose_oracle as O

G9_CASES = ["lsp_one", "lsp_two", "mpii_two_noise", "mpii_noise_peaks_raises", "posetrack_three", "ntid_one_rect",
            "lsp_plateau_raises", "lsp_missing_corner_raises", "lsp_empty_box_raises", "lsp_nothing"]
LSP_BATCH = ["lsp_one", "lsp_two", "lsp_plateau_raises", "lsp_missing_corner_raises", "lsp_empty_box_raises", "lsp_nothing"]
ERRORS = {"IndexError": IndexError, "ValueError": ValueError}
OK, MISSING, EMPTY, OVERFLOW = 0, 1, 2, 3
STATUS_OF = {IndexError: MISSING, ValueError: EMPTY}


def g9(golden_dir):
    return np.load(os.path.join(golden_dir, "g9_multi_person.npz"))


def dev_maps(maps, dev):
    return torch.from_numpy(np.ascontiguousarray(maps, dtype=np.float32)).to(dev)


def oracle(maps, ds="LSP"):
    """the list, or the exception type, of the numpy restatement on one sample (1, C, H, W)"""
    try:
        return O.unipose_kpts_multi(maps, ds)
    except (IndexError, ValueError) as e:
        return type(e)


def batch_lists(maps, dev, ds="LSP", **kw):
    from unipose_amd import ops
    return ops.uniPose_kpts_batch(dev_maps(maps, dev), ds, **kw)


def raw(maps, dev, ds="LSP", **kw):
    """ops.persons_decode -> numpy (kpts, count, status)"""
    from unipose_amd import ops
    return tuple(t.cpu().numpy() for t in ops.persons_decode(dev_maps(maps, dev), ds, **kw))


def as_list(kpts, count, b=0):
    """rows of sample b of a raw result in the reference's list form"""
    n = int(count[b])
    return [[p, int(x), int(y)] for p in range(n) for x, y in kpts[b, p].tolist()]


def against_oracle(maps, dev, ds="LSP", **kw):
    """one sample through the list form: the oracle's list, or its exception type; returns the oracle's outcome"""
    want = oracle(maps, ds)
    if isinstance(want, type):
        try:
            batch_lists(maps, dev, ds, **kw)
        except want:
            return want
        raise AssertionError(f"{want.__name__} expected")
    got = batch_lists(maps, dev, ds, **kw)
    assert got == [want], (got, want)
    return want


def nhwc_copy(maps, ld, dev):
    """the maps as a convolution leaves them: NHWC with `ld` physical channels, the pad channels filled with +inf"""
    b, c, h, w = maps.shape
    x = torch.full((b, h, w, ld), float("inf"), dtype=torch.float32)
    x[..., :c] = torch.from_numpy(maps).permute(0, 2, 3, 1)
    return x.to(dev)


def scene(h, w, peaks, seed=0, channels=20, f=15):
    """joint channels random, the five box maps -1 except the planted peaks: {map 0..4: [(row, col, value), ...]}"""
    rng = np.random.default_rng(seed)
    maps = rng.standard_normal((1, channels, h, w)).astype(np.float32)
    maps[0, f:f + 5] = -1.0
    for m, lst in peaks.items():
        for r, c, v in lst:
            maps[0, f + m, r, c] = v
    return maps


# 1 ---------------------------------------------------------------------------------------------------------------------------
def g9_case(dev, golden_dir, name):
    g = g9(golden_dir)
    maps, ds, err = g[name + "_maps"], str(g[name + "_dataset"]), str(g[name + "_error"])
    if name == "mpii_noise_peaks_raises":           # 235 centre peaks: overflow at the default 16, then the retry
        _, count, status = raw(maps, dev, ds)
        assert status.tolist() == [OVERFLOW] and count.tolist() == [235]
    if err:
        try:
            batch_lists(maps, dev, ds)
        except ERRORS[err]:
            return
        raise AssertionError(f"{err} expected")
    assert batch_lists(maps, dev, ds) == [g[name + "_kpts"].tolist()]


# 2 ---------------------------------------------------------------------------------------------------------------------------
def mixed_batch_case(dev, golden_dir):
    from unipose_amd import ops
    g = g9(golden_dir)
    maps = np.concatenate([g[n + "_maps"] for n in LSP_BATCH], 0)
    assert maps.shape == (6, 20, 46, 46)
    want_status = [OK, OK, MISSING, MISSING, EMPTY, OK]
    for b, n in enumerate(LSP_BATCH):                 # the expectation itself, against the fixture
        err = str(g[n + "_error"])
        assert want_status[b] == (STATUS_OF[ERRORS[err]] if err else OK)
    centres = [len(O.local_peaks(maps[b, 15])) for b in range(6)]
    assert centres[:3] == [1, 2, 4] and centres[5] == 0
    kpts, count, status = raw(maps, dev)
    assert status.tolist() == want_status and count.tolist() == centres
    for b in (0, 1, 5):
        assert as_list(kpts, count, b) == g[LSP_BATCH[b] + "_kpts"].tolist()
    lists = batch_lists(maps, dev, strict=False)
    assert [x is None for x in lists] == [False, False, True, True, True, False]
    for b in (0, 1, 5):
        assert lists[b] == g[LSP_BATCH[b] + "_kpts"].tolist()
    try:
        batch_lists(maps, dev)
        raise AssertionError("IndexError (sample 2) expected")
    except IndexError:
        pass
    got = tuple(t.cpu().numpy() for t in ops.persons_decode_nhwc(nhwc_copy(maps, 24, dev), 20, "LSP"))
    assert got[1].tolist() == centres and got[2].tolist() == want_status
    for b in (0, 1, 5):
        assert np.array_equal(got[0][b, :count[b]], kpts[b, :count[b]])


# 3 ---------------------------------------------------------------------------------------------------------------------------
def order_case(dev):
    """plateau pairs of centre peaks across a wavefront boundary (63 | 64) and a 256-pixel chunk boundary (255 | 256)"""
    from unipose_amd import ops
    peaks = {0: [(i // 20, i % 20, 2.0) for i in (63, 64, 255, 256, 399)],
             1: [(0, 2 * p, 1.0) for p in range(5)], 4: [(15, 10 + 2 * p, 1.0) for p in range(5)],
             2: [(3, 17, 1.0), (7, 1, 1.0), (9, 9, 1.0), (13, 5, 1.0), (18, 2, 1.0)],
             3: [(1, 1, 1.0), (5, 13, 1.0), (11, 3, 1.0), (16, 16, 1.0), (19, 0, 1.0)]}
    maps = scene(20, 20, peaks, seed=3)
    want = against_oracle(maps, dev)
    assert len(want) == 95
    assert [r[1:] for r in want[14::19]] == [[3, 3], [4, 3], [15, 12], [16, 12], [19, 19]]
    assert ops.uniPose_kpts(dev_maps(maps, dev), "LSP") == want


# 4 ---------------------------------------------------------------------------------------------------------------------------
def error_order_case(dev):
    centre = [(8, 8, 1.0), (16, 16, 1.0)]
    scenes = [
        # person 0: br[0] = (5, 5) is above tl[0] = (10, 10): empty box; person 1 has no bl
        ({0: centre, 1: [(10, 10, 1.0), (12, 2, 1.0)], 4: [(5, 5, 1.0), (20, 20, 1.0)], 2: [(20, 3, 1.0)],
          3: [(3, 20, 1.0), (6, 22, 1.0)]}, EMPTY, ValueError),
        # only one tl peak; person 1's br = (21, 1) would make an empty box with any tl to its right
        ({0: centre, 1: [(2, 2, 1.0)], 4: [(20, 20, 1.0), (21, 1, 1.0)], 2: [(20, 3, 1.0), (22, 5, 1.0)],
          3: [(3, 20, 1.0), (6, 22, 1.0)]}, MISSING, IndexError),
        # no bl peak at all; person 1: tl (15, 15), br (21, 3): empty box — person 0's bl check comes first
        ({0: centre, 1: [(2, 2, 1.0), (15, 15, 1.0)], 4: [(10, 10, 1.0), (21, 3, 1.0)], 2: [],
          3: [(3, 20, 1.0), (6, 22, 1.0)]}, MISSING, IndexError),
    ]
    batch = []
    for k, (peaks, status, err) in enumerate(scenes):
        maps = scene(24, 24, peaks, seed=10 + k)
        assert oracle(maps) is err
        assert against_oracle(maps, dev) is err
        _, count, st = raw(maps, dev)
        assert st.tolist() == [status] and count.tolist() == [2]
        batch.append(maps)
    _, count, st = raw(np.concatenate(batch, 0), dev)
    assert st.tolist() == [EMPTY, MISSING, MISSING] and count.tolist() == [2, 2, 2]


# 5 ---------------------------------------------------------------------------------------------------------------------------
def random_scenes_case(dev):
    """random boxes on random maps (after tests/test_multi_person.py): ties in one joint channel, error types included"""
    rng = np.random.default_rng(21)
    done = 0
    for trial in range(40):
        h, w = int(rng.integers(12, 40)), int(rng.integers(12, 40))
        n = int(rng.integers(1, 4))
        ys = np.sort(rng.choice(h - 1, size=2 * n, replace=False))
        xs = np.sort(rng.choice(w - 1, size=2 * n, replace=False))
        peaks = {m: [] for m in range(5)}
        for p in range(n):
            y0, y1, x0, x1 = (int(v) for v in (ys[2 * p], ys[2 * p + 1], xs[2 * p], xs[2 * p + 1]))
            for m, (yy, xx) in enumerate((((y0 + y1) // 2, (x0 + x1) // 2), (y0, x0), (y1, x0), (y0, x1), (y1, x1))):
                peaks[m].append((yy, xx, 1.0 + p))
        maps = scene(h, w, peaks, seed=100 + trial)
        maps[0, 3] = np.round(maps[0, 3])                       # many exact ties in one joint channel
        if not isinstance(against_oracle(maps, dev), type):
            done += 1
    assert done >= 10


# 6 ---------------------------------------------------------------------------------------------------------------------------
def edges_case(dev):
    # an 8 x 8 map: a single partial chunk
    small = scene(8, 8, {0: [(3, 3, 1.0)], 1: [(1, 1, 1.0)], 2: [(6, 1, 1.0)], 3: [(1, 6, 1.0)], 4: [(6, 6, 1.0)]}, seed=1)
    assert len(against_oracle(small, dev)) == 19
    # a 1 x 1 map: its only pixel is centre and every corner at once, the box is empty; and nothing at all
    one = np.ones((1, 20, 1, 1), np.float32)
    assert against_oracle(one, dev) is ValueError
    assert against_oracle(-one, dev) == []
    _, count, status = raw(np.concatenate([one, -one], 0), dev)
    assert count.tolist() == [1, 0] and status.tolist() == [EMPTY, OK]
    # peaks in all four corners of a map (12 x 13): four persons
    corners = scene(12, 13, {0: [(0, 0, 1.0), (0, 12, 1.0), (11, 0, 1.0), (11, 12, 1.0)],
                             1: [(0, 0, 1.0), (0, 3, 1.0), (1, 6, 1.0), (2, 1, 1.0)],
                             4: [(8, 4, 1.0), (9, 9, 1.0), (10, 8, 1.0), (11, 12, 1.0)],
                             2: [(11, 0, 1.0), (9, 2, 1.0), (7, 7, 1.0), (5, 5, 1.0)],
                             3: [(0, 12, 1.0), (2, 10, 1.0), (4, 8, 1.0), (6, 11, 1.0)]}, seed=2)
    assert len(against_oracle(corners, dev)) == 4 * 19
    # a corner map with more peaks than max_persons while the centre has 2: no overflow, the first two entries are used
    many = scene(16, 16, {0: [(4, 4, 1.0), (10, 10, 1.0)],
                          1: [(0, 0, 1.0), (1, 6, 1.0), (3, 12, 1.0), (8, 2, 1.0), (13, 13, 1.0)],
                          4: [(7, 5, 1.0), (12, 14, 1.0)], 2: [(7, 0, 1.0), (12, 6, 1.0)], 3: [(0, 5, 1.0), (1, 14, 1.0)]}, seed=3)
    kpts, count, status = raw(many, dev, max_persons=2)
    assert status.tolist() == [OK] and count.tolist() == [2]
    assert as_list(kpts, count) == oracle(many)
    # more centre peaks than the kernel's lists can hold (a plateau over the whole 24 x 24 map, 576 > 512): the raw call
    # reports overflow with the true count, the list form still gives the reference's outcome and keeps the neighbour
    flood = scene(24, 24, {}, seed=6)
    flood[0, 15:20] = 1.0
    _, count, status = raw(flood, dev, max_persons=512)
    assert count.tolist() == [576] and status.tolist() == [OVERFLOW]
    assert against_oracle(flood, dev) is ValueError
    other = scene(24, 24, {0: [(8, 8, 1.0)], 1: [(2, 3, 1.0)], 2: [(13, 3, 1.0)], 3: [(2, 12, 1.0)], 4: [(13, 12, 1.0)]}, seed=7)
    assert batch_lists(np.concatenate([flood, other], 0), dev, strict=False) == [None, oracle(other)]
    # inside a box: a joint channel holding NaN (the first NaN wins) and one holding only -inf (index 0 of the box)
    odd = scene(16, 16, {0: [(8, 8, 1.0)], 1: [(2, 3, 1.0)], 2: [(13, 3, 1.0)], 3: [(2, 12, 1.0)], 4: [(13, 12, 1.0)]}, seed=4)
    odd[0, 5, 9, 7] = odd[0, 5, 11, 4] = np.nan
    odd[0, 6] = -np.inf
    want = against_oracle(odd, dev)
    assert want[4] == [0, 7, 9] and want[5] == [0, 3, 2]
    # 128 x 160: five maps of 20480 values do not fit the LDS budget, the kernel reads through L2; three persons in the top-left
    # 40 x 60, whose crop (5 * 2400 values) takes the LDS path and must agree; a sixth tl peak far away is never used
    persons = {0: [(10, 10, 1.0), (20, 30, 2.0), (30, 50, 1.5)], 1: [(2, 3, 1.0), (12, 21, 1.0), (25, 41, 1.0)],
               4: [(18, 19, 1.0), (29, 40, 1.0), (38, 58, 1.0)], 2: [(18, 3, 1.0), (29, 21, 1.0), (38, 41, 1.0)],
               3: [(2, 19, 1.0), (12, 40, 1.0), (25, 58, 1.0)]}
    big = scene(128, 160, persons, seed=5)
    big[0, 16, 120, 150] = 1.0
    want = against_oracle(big, dev)
    assert len(want) == 57
    assert batch_lists(big[:, :, :40, :60], dev) == [want]


# 7 ---------------------------------------------------------------------------------------------------------------------------
def plan_case(dev, B):
    """the bbox model of tests/test_multi_person.py: K = 14, 64 x 64 input, 8 x 8 maps.  Synthetic weights: this proves the wiring
    and the NHWC read, the decode itself is proven by the cases above."""
    from model.unipose import unipose
    from unipose_amd import ops
    from unipose_amd.plan import UniPosePlan
    K = 14
    sd = O.synth_state_dict(K, 7)
    g = torch.Generator().manual_seed(3)
    sd["decoder.last_conv.8.weight"] = torch.randn(K + 6, 256, 1, 1, generator=g) * 0.05
    sd["decoder.last_conv.8.bias"] = torch.randn(K + 6, generator=g) * 0.1
    m = unipose("LSP", num_classes=K, bbox=True)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    x = O.synth_input((B, 3, 64, 64), 4).to(dev)
    plan = UniPosePlan(m, B, 64, 64)
    maps = torch.cat(plan(x), 1)
    assert maps.shape == (B, K + 6, 8, 8)
    want = tuple(t.cpu().numpy() for t in ops.persons_decode(maps, "LSP"))
    got = tuple(t.cpu().numpy() for t in plan.persons(x, "LSP"))
    print("plan.persons: count", got[1].tolist(), "status", got[2].tolist())
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    assert got[1].tolist() == [len(O.local_peaks(maps[b, 15].cpu().numpy())) for b in range(B)]
    for b in range(B):
        if got[2][b] == OK:
            assert np.array_equal(got[0][b, :got[1][b]], want[0][b, :want[1][b]])
    own = ops._persons_out(B, 16, 19, dev)[:3]
    assert all(a is o for a, o in zip(plan.persons(x, "LSP", out=own), own))
    assert own[1].cpu().tolist() == want[1].tolist() and own[2].cpu().tolist() == want[2].tolist()
    for bad in (dict(dataset="COCO"), dict(max_persons=0), dict(max_persons=ops.PERSONS_CAP + 1)):
        try:
            plan.persons(x, **{"dataset": "LSP", **bad})
            raise AssertionError(f"{bad} must be refused")
        except ValueError:
            pass
    try:
        plan.persons(x, "MPII")                       # box channels 17..21 of 20
        raise AssertionError("too few channels must be refused")
    except IndexError:
        pass
    plan.close()
    if B == 1:
        plain = unipose("LSP", num_classes=K)
        plain.load_state_dict(O.synth_state_dict(K, 7))
        p2 = UniPosePlan(plain.to(dev).eval(), 1, 64, 64)
        try:
            p2.persons(x, "LSP")
            raise AssertionError("a plan without the box head must be refused")
        except ValueError:
            pass
        p2.close()


def python_argument_case(dev):
    """the same ValueError / IndexError as ops.uniPose_kpts for an unknown dataset or too few channels"""
    from unipose_amd import ops
    z = torch.zeros(2, 20, 8, 8).to(dev)
    for fn in (ops.persons_decode, ops.uniPose_kpts_batch):
        for maps, ds, err in ((z, "COCO", ValueError), (z[:, :17], "LSP", IndexError), (z, "MPII", IndexError)):
            try:
                fn(maps, ds)
                raise AssertionError(f"{err.__name__} expected")
            except err:
                pass
    kpts, count, status = ops.persons_decode(z, "LSP", max_persons=3)
    assert kpts.shape == (2, 3, 19, 2) and kpts.dtype == count.dtype == status.dtype == torch.int32
    assert count.tolist() == [0, 0] and status.tolist() == [OK, OK]
    assert ops.uniPose_kpts_batch(z, "LSP") == [[], []]


# 8 ---------------------------------------------------------------------------------------------------------------------------
def c_abi_checks(dev):
    """every UP_ERR_INVALID condition of up_persons_decode and up_unipose_persons: refused before anything is launched"""
    from unipose_amd import _C
    from unipose_amd.plan import _Config
    L = _C.lib()
    buf = torch.zeros(4096).to(dev)
    p = buf.data_ptr()
    names = ("maps", "sb", "sj", "sp", "B", "C", "H", "W", "box", "joint", "nj", "mp", "count", "status", "kpts", "stream")
    ok = (p, 20 * 46 * 46, 46 * 46, 1, 1, 20, 46, 46, 15, 1, 14, 16, p, p, p, 0)

    def call(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return L.up_persons_decode(*[a[n] for n in names])

    for bad in (dict(maps=None), dict(count=None), dict(status=None), dict(kpts=None), dict(B=0), dict(C=0), dict(H=0), dict(W=-1),
                dict(sb=0), dict(sj=-1), dict(sp=0), dict(mp=0), dict(mp=513), dict(box=-1), dict(box=16), dict(joint=-1), dict(nj=0),
                dict(joint=7, nj=14), dict(sb=1 << 31, B=2), dict(sp=1 << 20), dict(sj=1 << 27), dict(B=1 << 16, mp=512)):
        assert call(**bad) == -1, bad
        assert L.up_last_error().startswith(b"persons_decode:"), (bad, L.up_last_error())
    plan = C.c_void_p()
    assert L.up_unipose_plan_create(C.byref(_Config(1, 64, 52, 16, 20)), C.byref(plan)) == 0
    names = ("plan", "x", "box", "joint", "nj", "mp", "count", "status", "kpts", "ws", "bytes", "stream")
    ok = (plan, p, 15, 1, 14, 16, p, p, p, p, 1 << 40, 0)

    def call_plan(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return L.up_unipose_persons(*[a[n] for n in names])

    assert call_plan() != 0 and b"never set" in L.up_last_error()         # legal arguments: the weights are what is missing
    for bad in (dict(plan=None), dict(x=None), dict(count=None), dict(status=None), dict(kpts=None), dict(ws=None), dict(box=-1),
                dict(box=16), dict(joint=-1), dict(nj=0), dict(joint=7, nj=14), dict(mp=0), dict(mp=513)):
        assert call_plan(**bad) == -1, bad
        assert L.up_last_error().startswith(b"unipose_persons:"), (bad, L.up_last_error())
    L.up_unipose_plan_destroy(plan)
