// shim/Sim3Solver_hip.h -- Sim3Solver with every RANSAC iteration on the device (shim/Sim3Solver_hip.cc; INTEGRATION.md, "Loop closing: Sim3Solver").
#ifndef ORBX_SHIM_SIM3SOLVER_HIP_H
#define ORBX_SHIM_SIM3SOLVER_HIP_H

#include <vector>

#include "Sim3Solver.h"

// Sim3Solver_hip.cc DEFINES the constructor, SetRansacParameters, iterate, find and the three getters of the reference's unmodified
// include/Sim3Solver.h: a build that links it leaves src/Sim3Solver.cc out.  A solver is solved - all mRansacMaxIts iterations, one device call -
// on its first iterate; iterate then replays the reference's stateful surface from the per-iteration results.
namespace orbx_shim
{
// Solves every solver of the list that has not been solved yet in ONE device call: what LoopClosing::ComputeSim3 calls once before its
// round-robin loop (src/LoopClosing.cc:403).  NULL entries (discarded candidates) are skipped.  false on a device error (shim_error.h).
bool SolveAll(const std::vector<ORB_SLAM2::Sim3Solver *> &solvers);
// Forgets what the shim keeps beside a solver (the reference's class has no destructor to hook): call before `delete pSolver`.
void Release(ORB_SLAM2::Sim3Solver *solver);
}  // namespace orbx_shim

// orbx_sim3_solve calls served so far / solvers they served (every thread)
extern "C" unsigned long orbx_shim_sim3_calls(void);
extern "C" unsigned long orbx_shim_sim3_solvers(void);

#endif
