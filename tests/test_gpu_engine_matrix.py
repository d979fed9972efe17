"""The generated scenes of tests/engine_matrix_cases.py on the GPU (pytest -m gpu): the generic kernel (GrxEngine<GrxShapeAny>, grx_point_step with agent = 1) takes one
step from each case's state, one world per case, and has to land where the live fp64 oracle lands -- the narrow-phase routines away from symmetric rest poses, free
joints under fast spin, and every size class of grx_sym_solve_full inside a real step (register-resident 14 .. 36, the two-block routes behind a trailing free body, the LDS route
next to them), and the row groups: welds, joint equalities, tendon limits and summed actuators, whose multi-entry spans feed the MFMA Hessian's operand fetch and whose
blocks the wave scans place between the limit and the contact rows).  Acceptance rule and caps: engine_matrix_cases.accept -- the same as on the emulator (tests/test_cpu_engine_matrix.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

import engine_matrix_cases as C

pytestmark = pytest.mark.gpu

RECORD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_matrix.json")))


def step_on_gpu(var):
    """one grx_point_step launch of the variant's model, one world per case; returns (x [n, nq + nv], status [n])"""
    import torch

    from gymnasium_robotics_amd import _native

    assert torch.cuda.is_available(), "these tests need the GPU"
    assert var.nq >= 2      # the step writes a two-word achieved goal and an observation of nq + nv - 2 words
    L, dev, n = _native.lib(), torch.device("cuda:0"), len(var.idx)
    H, I, F = var.model.pack()
    h = ctypes.c_void_p()
    _native.check(L.grx_model_create(H.ctypes.data, H.size, I.ctypes.data, I.size, F.ctypes.data, F.size, 0, ctypes.byref(h)))
    try:
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        z = lambda *sh, dtype=torch.float32: torch.zeros(*sh, dtype=dtype, device=dev)
        bufs = dict(qpos=f32(var.q0), qvel=f32(var.v0), qacc_ws=z(n, var.nv), goal=z(n, 2), action=f32(var.ctrl), obs=z(n, var.nq + var.nv), achieved=z(n, 2), reward=z(n),
                    success=z(n, dtype=torch.uint8), terminated=z(n, dtype=torch.uint8), status=z(n, dtype=torch.int32))
        b = _native.PointBuffersStruct()
        for k, t in bufs.items():
            setattr(b, k, t.data_ptr())
        b.mask = b.packed = None
        task = _native.PointTaskStruct(1, 1, 1, 1, 0.45, 5.0)       # agent = 1: ctrl = action, no velocity clip; one raw physics step
        _native.check(L.grx_point_step(h, ctypes.byref(task), ctypes.byref(b), n, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        torch.cuda.synchronize()
        x = np.concatenate([bufs["qpos"].cpu().numpy(), bufs["qvel"].cpu().numpy()], axis=1).astype(np.float64)
        return x, bufs["status"].cpu().numpy().astype(np.int64)
    finally:
        L.grx_model_destroy(h)


@pytest.mark.parametrize("name", C.NAMES)
def test_gpu_engine_equals_the_oracle(name):
    group = C.group(name)
    oracle = C.oracle_results(group)
    C.accept(group, [step_on_gpu(var) for var in group.variants], oracle, C.min_share(group, RECORD))
