// shim/ORBVocabulary_hip.h -- ORBVocabulary::create and ORBVocabulary::loadFromTextFile on the device (shim/ORBVocabulary_hip.cc).
#ifndef ORBX_SHIM_ORBVOCABULARY_HIP_H
#define ORBX_SHIM_ORBVOCABULARY_HIP_H

#include <string>
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
//
// loadFromTextFile(filename) HIDES the base's function (it is not virtual there): the text is indexed, parsed and turned into the tree on the
// device (orbx_vocabulary_load_text), m_nodes / m_words are filled from the flat arrays exactly as TemplatedVocabulary.h:1376-1420 leaves them,
// and the device handle stays with the object (Device()) for orbx_bow_transform* - no second flattening.  Stated differences: include/orbx.h
// (the empty last line of a file that ends in a newline is dropped; malformed files are refused: false, vocabulary empty).
class ORBVocabulary_hip : public ORBVocabulary
{
public:
    ORBVocabulary_hip(int k = 10, int L = 5, DBoW2::WeightingType weighting = DBoW2::TF_IDF, DBoW2::ScoringType scoring = DBoW2::L1_NORM,
                      int max_iterations = 100)
        : ORBVocabulary(k, L, weighting, scoring), mnMaxIterations(max_iterations), mnUnconverged(0), mpDevice(0)
    {
    }
    ~ORBVocabulary_hip();

    virtual void create(const std::vector<std::vector<DBoW2::FORB::TDescriptor> > &training_features, int k, int L, DBoW2::WeightingType weighting,
                        DBoW2::ScoringType scoring);

    bool loadFromTextFile(const std::string &filename);

    int UnconvergedNodes() const { return mnUnconverged; }      // nodes of the last create() that hit the cap
    orbx_vocabulary *Device() const { return mpDevice; }        // the device tree of the last successful loadFromTextFile (0 before), owned by this object

private:
    ORBVocabulary_hip(const ORBVocabulary_hip &);      // (owns a device handle)
    ORBVocabulary_hip &operator=(const ORBVocabulary_hip &);
    int mnMaxIterations, mnUnconverged;
    orbx_vocabulary *mpDevice;
};
}  // namespace ORB_SLAM2

#endif
