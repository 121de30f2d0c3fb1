// shim/ORBVocabulary_hip.h -- ORBVocabulary::create on the device (shim/ORBVocabulary_hip.cc).
#ifndef ORBX_SHIM_ORBVOCABULARY_HIP_H
#define ORBX_SHIM_ORBVOCABULARY_HIP_H

#include <vector>

#include "ORBVocabulary.h"
#include "orbx.h"

namespace ORB_SLAM2
{
// An ORBVocabulary whose create(training_features, k, L, weighting, scoring) runs on the device (orbx_voc_train).  Everything else -
// transform, score, save, load - is the reference's, on the m_nodes / m_words this fills.  A class of its own: the drop-in library
// keeps the reference's ORBVocabulary, and a tool that trains a vocabulary constructs this one.  The seed of the draws comes from the
// environment variable ORBX_VOC_SEED (default 0); max_iterations caps the assignment passes per node.  On a device error (shim_error.h)
// the vocabulary is left empty.
class ORBVocabulary_hip : public ORBVocabulary
{
public:
    ORBVocabulary_hip(int k = 10, int L = 5, DBoW2::WeightingType weighting = DBoW2::TF_IDF, DBoW2::ScoringType scoring = DBoW2::L1_NORM,
                      int max_iterations = 100)
        : ORBVocabulary(k, L, weighting, scoring), mnMaxIterations(max_iterations), mnUnconverged(0)
    {
    }

    virtual void create(const std::vector<std::vector<DBoW2::FORB::TDescriptor> > &training_features, int k, int L, DBoW2::WeightingType weighting,
                        DBoW2::ScoringType scoring);

    int UnconvergedNodes() const { return mnUnconverged; }      // nodes of the last create() that hit the cap

private:
    int mnMaxIterations, mnUnconverged;
};
}  // namespace ORB_SLAM2

#endif
