"""What the wrapper classes share through _Handle (Python) and OrbxHandle / OrbxCallTimer (csrc/orbx_handle.h), pinned per class: the
constructor without a device, create / close / close, destruction in either order, a device index out of range, and what last_timing()
says on a handle that never ran - the one point where the handles differ on purpose ("Handles")."""
import ctypes

import numpy as np
import pytest

ERR_ARG, ERR_NODEVICE, ERR_STATE = -1, -4, -5
STATE, ZEROS = "ORBX_ERR_STATE", "zeros"

_VOC = dict(k=2, L=1, parent=np.zeros(3, np.int32), is_leaf=np.array([0, 1, 1], np.uint8), desc=np.zeros((3, 32), np.uint8), weight=np.array([0.0, 1.0, 1.0]))
_KEEP = []      # arrays and structures the raw create calls point into


def _cfg(S, *a):
    _KEEP.append(S(*a))
    return ctypes.byref(_KEEP[-1])


def _voc_raw(L, d, out):
    v = {k: np.ascontiguousarray(x) for k, x in _VOC.items() if k not in ("k", "L")}
    _KEEP.append(v)
    return L.orbx_vocabulary_create(d, 2, 1, 3, *(ctypes.c_void_p(v[k].ctypes.data) for k in ("parent", "is_leaf", "desc", "weight")), out)


# class name: (constructor with its smallest legal arguments, the raw *_create with the same ones, last_timing() of a handle that never ran)
CASES = {
    # (the extractor at a size the suite uses elsewhere: its lifecycle - streams, combiner - is its own)
    "ORBextractor": (lambda o, d: o.ORBextractor(500, 1.2, 8, 20, 7, max_width=400, max_height=300, device=d),
                     lambda o, L, d, out: L.orbx_extractor_create(_cfg(o.ExtractorConfig, 500, 1.2, 8, 20, 7, 400, 300, 1, d), out), None),
    "ORBmatcher": (lambda o, d: o.ORBmatcher(max_features=1, max_pairs=1, device=d), lambda o, L, d, out: L.orbx_matcher_create(d, 1, 1, out), None),
    "Vocabulary": (lambda o, d: o.Vocabulary(_VOC, device=d), lambda o, L, d, out: _voc_raw(L, d, out), None),
    "VocabularyTrainer": (lambda o, d: o.VocabularyTrainer(2, 1, 1, 1, device=d), lambda o, L, d, out: L.orbx_voc_trainer_create(d, 2, 1, 1, 1, out), None),
    "FrameOps": (lambda o, d: o.FrameOps(1.0, 1.0, 0.0, 0.0, [0.0] * 4, device=d),
                 lambda o, L, d, out: L.orbx_frame_ops_create(d, _cfg(o.Camera, 1.0, 1.0, 0.0, 0.0, (ctypes.c_float * 5)(), 4), out), None),
    "PoseOptimizer": (lambda o, d: o.PoseOptimizer(1, 1, device=d), lambda o, L, d, out: L.orbx_pose_optimizer_create(d, 1, 1, out), None),
    "Optimizer": (lambda o, d: o.Optimizer(1, 1, 1, device=d), lambda o, L, d, out: L.orbx_lba_create(d, 1, 1, 1, out), STATE),
    "BatchOptimizer": (lambda o, d: o.BatchOptimizer(1, 1, 1, 1, device=d), lambda o, L, d, out: L.orbx_lba_batch_create(d, 1, 1, 1, 1, out), STATE),
    "MapPointOps": (lambda o, d: o.MapPointOps(1, 1, device=d), lambda o, L, d, out: L.orbx_mappoint_ops_create(d, 1, 1, out), ZEROS),
    "Initializer": (lambda o, d: o.Initializer(iterations=1, max_matches=8, device=d), lambda o, L, d, out: L.orbx_initializer_create(d, 8, 1, out), STATE),
    "Sim3Solver": (lambda o, d: o.Sim3Solver(1, 3, 1, device=d), lambda o, L, d, out: L.orbx_sim3_solver_create(d, 1, 3, 1, out), STATE),
    "Sim3Optimizer": (lambda o, d: o.Sim3Optimizer(1, 1, device=d), lambda o, L, d, out: L.orbx_sim3_optimizer_create(d, 1, 1, out), STATE),
    "PnPsolver": (lambda o, d: o.PnPsolver(1, 4, 1, device=d), lambda o, L, d, out: L.orbx_pnp_solver_create(d, 1, 4, 1, out), STATE),
    "EssentialGraphOptimizer": (lambda o, d: o.EssentialGraphOptimizer(1, 0, device=d), lambda o, L, d, out: L.orbx_essential_graph_create(d, 1, 0, 0, 1, out), STATE),
    "KeyFrameDatabase": (lambda o, d: o.KeyFrameDatabase(1, 1, 1, 1, 1, device=d), lambda o, L, d, out: L.orbx_kfdb_create(d, 1, 1, 1, 1, 1, out), ZEROS),
    "Covisibility": (lambda o, d: o.Covisibility(device=d), lambda o, L, d, out: L.orbx_covis_create(d, out), ZEROS),
    "LoopCorrection": (lambda o, d: o.LoopCorrection(device=d), lambda o, L, d, out: L.orbx_loop_create(d, out), ZEROS),
    "ImagePrep": (lambda o, d: o.ImagePrep(1, 1, 1, device=d), lambda o, L, d, out: L.orbx_image_prep_create(_cfg(o.ImagePrepConfig, d, 1, 1, 1), out), ZEROS),
}
NAMES = sorted(CASES)


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_every_wrapper_class_is_a_case(orbx):
    derived = {n for n, c in vars(orbx).items() if isinstance(c, type) and issubclass(c, orbx._Handle) and c is not orbx._Handle}
    assert derived == set(CASES)
    for n in derived:
        assert hasattr(orbx.load_library(), getattr(orbx, n)._destroy), n


@pytest.mark.parametrize("name", NAMES)
def test_constructor_without_a_device(orbx, name):
    """ORBX_ERR_NODEVICE without a device (no CPU fallback); a handle with one"""
    if _gpu():
        CASES[name][0](orbx, 0).close()
        return
    with pytest.raises(orbx.OrbxError) as e:
        CASES[name][0](orbx, 0)
    assert e.value.code == ERR_NODEVICE


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_create_close_close(orbx, name):
    h = CASES[name][0](orbx, 0)
    assert h._h and h._L is orbx.load_library()
    h.close()
    left = h._h
    assert not left and (isinstance(left, ctypes.c_void_p) if type(h)._keeps_pointer else left is None)
    h.close()
    assert type(h._h) is type(left) and not h._h


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_two_handles_destroyed_in_either_order(orbx, name):
    make = CASES[name][0]
    a, b = make(orbx, 0), make(orbx, 0)
    assert a._h.value != b._h.value
    a.close(); b.close()
    a, b = make(orbx, 0), make(orbx, 0)
    b.close(); a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_out_of_range(orbx, name):
    import torch
    make, raw, _ = CASES[name]
    ndev = torch.cuda.device_count()
    make(orbx, 0).close()      # (binds the argument types of the class's symbols)
    with pytest.raises(orbx.OrbxError) as e:
        make(orbx, ndev)
    assert e.value.code == ERR_ARG
    out = ctypes.c_void_p(0xdead0)
    assert raw(orbx, orbx.load_library(), ndev, ctypes.byref(out)) == ERR_ARG
    assert not out.value
    _KEEP.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in NAMES if CASES[n][2]])
def test_last_timing_of_a_handle_that_never_ran(orbx, name):
    h = CASES[name][0](orbx, 0)
    try:
        if CASES[name][2] == STATE:
            with pytest.raises(orbx.OrbxError) as e:
                h.last_timing()
            assert e.value.code == ERR_STATE
        else:
            assert h.last_timing() == (0.0, 0)
    finally:
        h.close()


@pytest.mark.gpu
def test_new_points_last_timing_of_a_matcher_that_never_ran(orbx):
    m = orbx.ORBmatcher(max_features=1, max_pairs=1)
    try:
        with pytest.raises(orbx.OrbxError) as e:
            m.new_points_last_timing()
        assert e.value.code == ERR_STATE
    finally:
        m.close()
