"""Host half of the native step runtime (no GPU): record validation in gcl_plan_create, the dry-run arena sizing of
gcl_maps_arena_bytes / gcl_plan_arena_bytes, and the bucket segmentation of NetworkPlan."""
import ctypes

import pytest

from gcl_amd import _lib


def _op(**kw):
    d = dict(kind=0, x=-1, x2=-1, y=-1, level_in=0, level_out=0, cin=0, cout=0, map=-1, transpose=0, K=1, w=-1, bias=-1,
             bn_w=-1, bn_b=-1, bn=-1, relu=0, momentum=0.0, eps=1e-5)
    d.update(kw)
    return d


def _mini_records():
    """stem convbn -> convbn 3^3 (relu) -> convbn 3^3 (+ residual, relu) -> stride-2 convbn -> transposed convbn ->
    cat -> 1x1 conv -> relu -> 1x1 conv + bias -> rownorm"""
    C = _lib.OP_CONVBN
    return [
        _op(kind=C, x=0, y=1, cin=1, cout=32, map=0, K=125, w=0, bn_w=1, bn_b=2, bn=0),
        _op(kind=C, x=1, y=2, cin=32, cout=32, map=1, K=27, w=3, bn_w=4, bn_b=5, bn=1, relu=1),
        _op(kind=C, x=2, x2=1, y=3, cin=32, cout=32, map=1, K=27, w=6, bn_w=7, bn_b=8, bn=2, relu=1),
        _op(kind=C, x=3, y=4, level_out=1, cin=32, cout=64, map=2, K=27, w=9, bn_w=10, bn_b=11, bn=3, relu=1),
        _op(kind=C, x=4, y=5, level_in=1, level_out=0, cin=64, cout=32, map=2, transpose=1, K=27, w=12, bn_w=13, bn_b=14,
            bn=4, relu=1),
        _op(kind=_lib.OP_CAT, x=5, x2=3, y=6, cin=32, cout=64),
        _op(kind=_lib.OP_CONV, x=6, y=7, cin=64, cout=64, map=3, K=1, w=15),
        _op(kind=_lib.OP_RELU, x=7, y=8, cin=64, cout=64),
        _op(kind=_lib.OP_CONV, x=8, y=9, cin=64, cout=32, map=3, K=1, w=16, bias=17),
        _op(kind=_lib.OP_ROWNORM, x=9, y=10, cin=32, cout=32),
    ]


def _create(records, n_tensors=11, n_params=18, worder=(3, 6, 9, 12, 15, 16), presplit=128):
    lib = _lib.load()
    arr = (_lib.PlanOp * len(records))()
    for a, r in zip(arr, records):
        for k, v in r.items():
            setattr(a, k, v)
    wo = (ctypes.c_int32 * max(1, len(worder)))(*worder)
    return lib.gcl_plan_create(arr, len(records), n_tensors, n_params, wo, len(worder), presplit)


def _maps(n=10000, n1=3000):
    d = _lib.MapsDesc()
    d.n_levels, d.n_maps = 2, 4
    d.n_rows[0], d.n_rows[1] = n, n1
    for i, (t, ks, st, li, lo) in enumerate([(1, 5, 1, 0, 0), (1, 3, 1, 0, 0), (1, 3, 2, 0, 1), (1, 1, 1, 0, 0)]):
        m = d.maps[i]
        m.t_in, m.kernel_size, m.stride, m.K, m.level_in, m.level_out = t, ks, st, ks ** 3, li, lo
        m.n_in, m.n_out = d.n_rows[li], d.n_rows[lo]
        m.n_pairs = 8 * m.n_out
        for k in range(m.K + 1):
            m.seg_off[k] = k * 1024
    return d


def test_plan_create_accepts_a_resunet_shaped_graph_and_sizes_its_arena():
    lib = _lib.load()
    h = _create(_mini_records())
    assert h, lib.gcl_last_error()
    h = ctypes.c_void_p(h)
    assert lib.gcl_plan_state_bytes(h) >= 6 * 18 * 8
    d = _maps()
    small = lib.gcl_plan_arena_bytes(h, ctypes.byref(d))
    big = lib.gcl_plan_arena_bytes(h, ctypes.byref(_maps(20000, 6000)))
    # activations alone: 10 k rows x (32 * 7 + 64 * 4) floats forward, and at least as much again backward
    assert small > 10000 * 4 * (32 * 7 + 64 * 4) and 1.8 * small < big < 2.2 * small
    d.maps[2].level_out = 0          # the records and the maps must agree on the levels
    assert lib.gcl_plan_arena_bytes(h, ctypes.byref(d)) < 0 and b"levels" in lib.gcl_last_error()
    # without a GPU the forward entry still validates its arguments before any HIP call
    assert lib.gcl_plan_forward(h, None, None, None, None, None, None, 0, None, None) == -1
    assert lib.gcl_plan_backward(h, None, None, (ctypes.c_void_p * 18)(), 0, 10, None) == -1
    assert b"no forward pass" in lib.gcl_last_error()
    lib.gcl_plan_destroy(h)


# (gcl_plan_arena_bytes, gcl_plan_eval_arena_bytes) for _maps(10000, 3000) and for _maps(300, 100), as returned by the library
# of commit 5445072 ("Head forward: run the row-local records on the rows the loss reads") cross-compiled for gfx950.  The dry
# sizing walks every record's forward and backward body, the touched-row suffix on the largest list included, so a moved,
# added or lost arena allocation in any of them changes a number here.
_ARENA_PINS = {
    "full": ((45784320, 15055936), (4207744, 617136)),
    "no_rownorm": ((43151616, 13723648), (4116608, 565248)),      # rec[:9]: the suffix is three records
    "no_suffix": ((27608064, 7274496), (3536000, 324096)),        # rec[:5]
    "presplit_64": ((53758464, 20175936), (4451200, 770736)),     # the head's widths read plane images
}


@pytest.mark.parametrize("case", sorted(_ARENA_PINS))
def test_arena_sizes_are_the_ones_the_dense_and_touched_row_bodies_took_before_they_were_shared(case):
    lib = _lib.load()
    rec = _mini_records()
    kw = dict(n_tensors=11, n_params=18, worder=(3, 6, 9, 12, 15, 16))
    if case == "no_rownorm":
        rec, kw["n_tensors"] = rec[:9], 10
    elif case == "no_suffix":
        rec, kw = rec[:5], dict(n_tensors=6, n_params=15, worder=(3, 6, 9, 12))
    h = _create(rec, presplit=64 if case == "presplit_64" else 128, **kw)
    assert h, lib.gcl_last_error()
    h = ctypes.c_void_p(h)
    for (n, n1), want in zip(((10000, 3000), (300, 100)), _ARENA_PINS[case]):
        d = _maps(n, n1)
        got = (lib.gcl_plan_arena_bytes(h, ctypes.byref(d)), lib.gcl_plan_eval_arena_bytes(h, ctypes.byref(d)))
        assert got == want, (case, n, got, want)
    lib.gcl_plan_destroy(h)


def _graph_variant(case):
    """_mini_records() with one edit per graph analysis of gcl_plan_create whose condition the edit flips."""
    r = _mini_records()
    kw = {}
    if case in ("g_wide", "h_wide_cat_swapped"):      # every width x 4 (the stem keeps its one input channel): bound mode
        for o in r:
            o.update(cin=o["cin"] * 4 if o["cin"] > 1 else 1, cout=o["cout"] * 4)
    if case == "a_conv_read_twice":            # the 1x1 conv's output has a second reader: no ReLU in its epilogue
        r[8].update(x=7)
    elif case == "b_cat_left_read_twice":      # the cat's left input has a second reader: no cat in place
        r[6].update(x=5, cin=32)
    elif case in ("c_cat_swapped", "h_wide_cat_swapped"):
        r[5]["x"], r[5]["x2"] = r[5]["x2"], r[5]["x"]
    elif case == "d_relu_read_twice":          # the ReLU has two readers: no mask_from, and the suffix moves
        r[9].update(x=8, cin=64, cout=64)
    elif case == "e_ends_in_relu":
        r, kw = r[:8], dict(n_tensors=9, n_params=16, worder=(3, 6, 9, 12, 15))
    elif case == "f_ends_in_conv":
        r, kw = r[:7], dict(n_tensors=8, n_params=16, worder=(3, 6, 9, 12, 15))
    return r, kw


# case -> presplit -> (touched suffix, plane-only flags, (arena, eval arena) at _maps(10000, 3000), the same at _maps(300, 100)),
# as returned by the library of commit 1a22491 ("Loss backward without float atomics: opt-in bitwise-reproducible steps")
# cross-compiled for gfx950: what fuse_relu, cat_left, mask_from, the suffix search and the plane-only analysis decided from the
# records before they shared one reader table.  "base" is _mini_records() itself; every variant differs from it.
_GRAPH_PINS = {
    "base": {
        128: (6, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], (45784320, 15055936), (4207744, 617136)),
        64: (6, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], (53758464, 20175936), (4451200, 770736)),
    },
    "a_conv_read_twice": {
        128: (9, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], (49042176, 17615936), (4297856, 693936)),
        64: (9, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], (58258688, 22735936), (4579968, 847536)),
    },
    "b_cat_left_read_twice": {
        128: (7, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], (45760256, 15055936), (4183680, 617136)),
        64: (7, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], (52416768, 17615936), (4388992, 693936)),
    },
    "c_cat_swapped": {
        128: (6, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], (47064320, 15055936), (4246144, 617136)),
        64: (6, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], (55038464, 20175936), (4489600, 770736)),
    },
    "d_relu_read_twice": {
        128: (10, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], (45695232, 16335936), (4194688, 655536)),
        64: (10, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], (54911744, 21455936), (4476800, 809136)),
    },
    "e_ends_in_relu": {
        128: (6, [0, 0, 0, 0, 0, 0, 0, 0], (41772800, 12431360), (4039552, 514560)),
        64: (6, [0, 0, 0, 0, 0, 0, 0, 0], (47149056, 14991360), (4206208, 591360)),
    },
    "f_ends_in_conv": {
        128: (6, [0, 0, 0, 0, 0, 0, 0], (39201024, 12419072), (3950976, 502272)),
        64: (6, [0, 0, 0, 0, 0, 0, 0], (44577280, 14979072), (4117632, 579072)),
    },
    "g_wide": {
        128: (6, [0, 3, 0, 3, 0, 0, 0, 0, 0, 0], (251622144, 80079936), (50534656, 2575536)),
        64: (6, [0, 3, 0, 3, 0, 0, 0, 0, 0, 0], (251622144, 80079936), (50534656, 2575536)),
    },
    "h_wide_cat_swapped": {
        128: (6, [0, 3, 0, 3, 0, 0, 0, 0, 0, 0], (261862144, 80079936), (50841856, 2575536)),
        64: (6, [0, 3, 0, 3, 0, 0, 0, 0, 0, 0], (261862144, 80079936), (50841856, 2575536)),
    },
}


@pytest.mark.parametrize("presplit", [128, 64])
@pytest.mark.parametrize("case", ["base", "a_conv_read_twice", "b_cat_left_read_twice", "c_cat_swapped", "d_relu_read_twice",
                                  "e_ends_in_relu", "f_ends_in_conv", "g_wide", "h_wide_cat_swapped"])
def test_graph_analyses_decide_what_they_decided_before_the_reader_table(case, presplit):
    lib = _lib.load()
    rec, kw = _graph_variant(case)
    h = _create(rec, presplit=presplit, **kw)
    assert h, lib.gcl_last_error()
    h = ctypes.c_void_p(h)
    flags = (ctypes.c_int32 * len(rec))()
    assert lib.gcl_plan_plane_only(h, flags, len(rec)) >= 0
    got = (lib.gcl_plan_touched_suffix(h), list(flags)) + tuple(
        (lib.gcl_plan_arena_bytes(h, ctypes.byref(d)), lib.gcl_plan_eval_arena_bytes(h, ctypes.byref(d)))
        for d in (_maps(10000, 3000), _maps(300, 100)))
    lib.gcl_plan_destroy(h)
    assert got == _GRAPH_PINS[case][presplit], (case, presplit, got)
    assert case == "base" or got != _GRAPH_PINS["base"][presplit]


@pytest.mark.parametrize("mutate,why", [
    (lambda r: r[1].update(x=5), "consumes a tensor produced later"),
    (lambda r: r[2].update(w=3), "one parameter in two records (gradients are written, not added)"),
    (lambda r: r[6].update(cout=48), "generic shapes stay on the per-operator path"),
    (lambda r: r[5].update(x2=-1), "cat needs two inputs"),
    (lambda r: r[8].update(kind=_lib.OP_CONVBN), "bias with BatchNorm"),
    (lambda r: r[0].update(kind=9), "unknown kind"),
])
def test_plan_create_rejects_malformed_graphs(mutate, why):
    rec = _mini_records()
    mutate(rec)
    assert not _create(rec), why
    assert b"gcl_plan_create" in _lib.load().gcl_last_error()


def test_maps_arena_bound_grows_with_the_cloud_and_covers_every_spec():
    lib = _lib.load()
    specs = [(1, 5, 1, 0, 0), (1, 3, 1, 1, 1), (1, 3, 2, 3, 1), (2, 3, 1, 1, 1), (1, 1, 1, 0, 1)]
    arr = (_lib.MapSpec * len(specs))()
    for a, s in zip(arr, specs):
        a.t_in, a.kernel_size, a.stride, a.tables, a.pairs = s
    a = lib.gcl_maps_arena_bytes(100000, arr, len(specs), 4)
    b = lib.gcl_maps_arena_bytes(200000, arr, len(specs), 4)
    assert a > 100000 * 4 * (125 + 2 * 27 * 3) and 1.7 * a < b < 2.3 * a
    assert lib.gcl_maps_arena_bytes(0, arr, len(specs), 4) < 0
    arr[2].t_in = 16                                # outside the 4 levels
    assert lib.gcl_maps_arena_bytes(1000, arr, len(specs), 4) < 0


def test_bucket_segments_follow_the_lowest_record_of_each_bucket():
    from gcl_amd.MinkowskiEngine.native import NetworkPlan
    plan = NetworkPlan.__new__(NetworkPlan)
    plan.handle = None
    plan.records = _mini_records()
    plan.bucket_of_param, plan.on_bucket = None, None
    assert plan._segments() == [(0, 10, [])]
    # parameters 0..8 (records 0-2) in bucket 0, the rest in bucket 1: bucket 1 is complete once record 3 has run
    plan.bucket_of_param = {p: (0 if p < 9 else 1) for p in range(18)}
    plan.on_bucket = lambda b: None
    assert plan._segments() == [(3, 10, [1]), (0, 3, [0])]
