// orbx_optsim3.h -- what a chain of another file needs to run k_optsim3 (orbx_optimize_sim3.hip) as one of its links: the problem header, the layout of
// a problem's result block, the kernel's input view and the enqueue.  The build has no relocatable device code, so the kernel stays in its file.
#ifndef ORBX_OPTSIM3_H
#define ORBX_OPTSIM3_H

#include "orbx_handle.h"
#include "orbx_sim3_group.h"

struct OsProb {                  // one problem of a call: in mapped pinned memory, host-filled (orbx_optimize_sim3), or in device memory, filled by k_ls_mutual
    float rcw1[9], tcw1[3], rcw2[9], tcw2[3];
    float k1[4], k2[4];          // fx, fy, cx, cy
    double r12[9], t12[3], s12;
    float th2;
    int32_t n, fixScale, mb;     // mb: first pair of this problem in the call's arrays
    unsigned long long outOff;   // the problem's result block in the mapped result buffer
};
static_assert(sizeof(OsProb) % 8 == 0, "holds 8-byte members");

struct OsBlock {                 // layout of a problem's result block (mapped pinned); head = {n_inliers, n_bad, 0, 0}
    size_t est, stats, r12, remFirst, remFinal, chi1, chi2, x1, x2, total;
    __host__ __device__ OsBlock(int n)
    {
        const size_t m = (size_t)n, m8 = (m + 7) & ~(size_t)7;
        est = 16; stats = est + 64; r12 = stats + 32; remFirst = r12 + 40; remFinal = remFirst + m8; chi1 = remFinal + m8; chi2 = chi1 + 16 * m;
        x1 = chi2 + 16 * m; x2 = x1 + 12 * m;
        total = (x2 + 12 * m + 255) & ~(size_t)255;
    }
};

struct OsIn {                    // the call's inputs: device addresses of mapped pinned memory, or device memory (a chain)
    const OsProb *prob;
    const float *world1, *world2, *obs1, *obs2, *inv1, *inv2;
    const uint8_t *active;       // LIN: [n] or nullptr = every pair
    OsSim3 lin;                  // LIN: the estimate
};

/* k_optsim3 for `np` problems in ONE launch on `st`, the instantiation that holds maxN pairs per problem (the host's bound; a problem's own n is read from
 * its header, and n = 0 returns at once with n_inliers = 0 and the input estimate).  I.prob, the pair arrays and `out` may be mapped host memory
 * (orbx_optimize_sim3) or device memory that an earlier kernel of the chain filled (orbx_loop_sim3.hip).  The last workgroup to finish stores `seq` to
 * *flag behind everybody's results; counter: a device word that is 0 between launches.  The caller checks the launch. */
void orbx_optsim3_enqueue(hipStream_t st, const OsIn &I, uint8_t *out, int np, int maxN, unsigned *counter, unsigned long long *flag, unsigned long long seq);

#endif
