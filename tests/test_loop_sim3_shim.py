"""shim/ComputeSim3_hip.{h,cc}: the binding of orbx_loop_refine_sim3 to real KeyFrame / MapPoint objects compiles against the reference's headers
(-fsyntax-only: nothing linked, nothing run), makes the call it claims and stays out of the drop-in library.  Needs the reference sources."""
import os
import subprocess
import tempfile
from pathlib import Path

import pytest

from test_callers_compile import REF, ROOT

SHIM = ROOT / "self_commit_orb-slam2_amd" / "shim"


@pytest.mark.skipif(not os.access(REF / "include" / "LoopClosing.h", os.R_OK), reason="the reference sources are not readable here")
def test_shim_compiles_against_the_reference_headers():
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "a" / "b").mkdir(parents=True)
        (Path(d) / "config.h").write_bytes((ROOT / "oracle" / "eigenshim" / "config.h").read_bytes())      # g2o's "../../config.h"
        cmd = ["g++", "-std=gnu++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-Wall", "-w", "-fvisibility=hidden",
               "-I" + str(ROOT / "oracle" / "cvshim"), "-I" + str(ROOT / "oracle" / "eigenshim"), "-I" + str(Path(d) / "a" / "b"), "-I" + str(REF), "-I" + str(REF / "include"),
               "-DORBSLAM_HIP", "-include", str(REF / "include" / "Tracking.h"), "-I" + str(ROOT / "include"), "-fsyntax-only", str(SHIM / "ComputeSim3_hip.cc")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shim_makes_the_call_it_claims_and_is_not_linked_into_the_drop_in_library():
    text = (SHIM / "ComputeSim3_hip.cc").read_text()
    for piece in ("orbx_loop_refine_sim3(", "A.Gather(pKF, true)", "ORBX_LOOP_SIM3_MAX_HYPOTHESES", "shim_error.h", "orbx_shim::Fail(", "orbx_predict_scale_thresholds(",
                  "mnMinX", "gScm * g2o::Sim3("):
        assert piece in text, piece
    assert text.count("orbx_loop_refine_sim3(") == 1
    assert "MapPointAccess::Snapshot(" in (SHIM / "KeyFrameArrays.h").read_text() and "withPointData" in (SHIM / "KeyFrameArrays.h").read_text()
    assert "ComputeSim3Device" in (SHIM / "ComputeSim3_hip.h").read_text()
    assert "ComputeSim3_hip" not in (ROOT / "oracle" / "Makefile").read_text()
    assert "ComputeSim3_hip" in (ROOT / "INTEGRATION.md").read_text()
