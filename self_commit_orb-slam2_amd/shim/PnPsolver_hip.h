// shim/PnPsolver_hip.h -- PnPsolver with every RANSAC iteration and every Refine on the device (shim/PnPsolver_hip.cc; INTEGRATION.md, "Relocalisation: PnPsolver").
#ifndef ORBX_SHIM_PNPSOLVER_HIP_H
#define ORBX_SHIM_PNPSOLVER_HIP_H

#include <vector>

#include "PnPsolver.h"

// PnPsolver_hip.cc DEFINES the constructor, the destructor, SetRansacParameters, iterate and find of the reference's unmodified
// include/PnPsolver.h: a build that links it leaves src/PnPsolver.cc out (the EPnP members are not defined: nothing calls them).  A solver is
// solved - all mRansacMaxIts iterations and the Refine of every record, one device call - on its first iterate; iterate then replays the
// reference's stateful surface from the per-iteration and per-record results.
namespace orbx_shim
{
// Solves every solver of the list that has not been solved yet in ONE device call: what Tracking::Relocalization calls once before its
// round-robin loop (src/Tracking.cc, behind the SearchByBoW loop).  NULL entries (discarded candidates) are skipped.  false on a device
// error (shim_error.h).
bool SolveAll(const std::vector<ORB_SLAM2::PnPsolver *> &solvers);
// Forgets what the shim keeps beside a solver; the destructor does the same, so a caller that deletes its solvers need not call it.
void Release(ORB_SLAM2::PnPsolver *solver);
}  // namespace orbx_shim

// orbx_pnp_solve calls served so far / solvers they served (every thread)
extern "C" unsigned long orbx_shim_pnp_calls(void);
extern "C" unsigned long orbx_shim_pnp_solvers(void);

#endif
