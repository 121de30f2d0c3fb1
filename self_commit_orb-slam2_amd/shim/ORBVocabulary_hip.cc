// shim/ORBVocabulary_hip.cc -- TemplatedVocabulary::create(training_features, k, L, weighting, scoring)
// (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:604-616 over :557-587) through orbx_voc_train.
//
// Compiled against the REFERENCE's own headers, like the other shim files.  A file of its own: the drop-in library of oracle/Makefile does not
// link it; it is compile-checked only.
//
// What stays on the host: gathering the rows of the cv::Mat descriptors (one 1 x 32 CV_8U row each, image after image, as getFeatures walks
// them), and filling m_nodes (descriptor, parent, children, weight, word_id) and m_words from the flat arrays, whose node and word ids are
// the ones HKmeansStep and createWords hand out.  The draws are the library's counter hash, not rand(): PARITY UNPINNED against the
// reference's rand() order, as are the empty-cluster rule and the cap (include/orbx.h).  On a device error (counted, std::cerr:
// shim_error.h) the vocabulary is left empty.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ORBVocabulary.h"
#include "orbx.h"
#include "shim_error.h"
#include "ORBVocabulary_hip.h"

namespace ORB_SLAM2
{
void ORBVocabulary_hip::create(const std::vector<std::vector<DBoW2::FORB::TDescriptor> > &training_features, int k, int L, DBoW2::WeightingType weighting,
                               DBoW2::ScoringType scoring)
{
    m_k = k;
    m_L = L;
    m_weighting = weighting;
    m_scoring = scoring;
    createScoringObject();
    m_nodes.clear();
    m_words.clear();
    mnUnconverged = 0;

    std::vector<int32_t> counts;
    std::vector<uint8_t> bytes;
    size_t total = 0;
    for (size_t i = 0; i < training_features.size(); i++) total += training_features[i].size();
    counts.reserve(training_features.size());
    bytes.reserve(total * 32);
    for (size_t i = 0; i < training_features.size(); i++) {
        counts.push_back((int32_t)training_features[i].size());
        for (size_t j = 0; j < training_features[i].size(); j++) {
            const cv::Mat &d = training_features[i][j];
            if (d.rows != 1 || d.cols != 32 || d.type() != CV_8U) { orbx_shim::Fail("ORBVocabulary::create", "a descriptor is not a 1 x 32 CV_8U row"); return; }
            const unsigned char *p = d.ptr<unsigned char>();
            bytes.insert(bytes.end(), p, p + 32);
        }
    }
    m_nodes.push_back(Node(0));      // root
    if (total == 0) return;          // (HKmeansStep returns at once on an empty set: the root alone)

    const char *env = getenv("ORBX_VOC_SEED");
    orbx_voc_train_params params;
    params.seed = env ? strtoull(env, 0, 10) : 0;
    params.weighting = (int)weighting;      // DBoW2::WeightingType: TF_IDF, TF, IDF, BINARY = 0 .. 3
    params.max_iterations = mnMaxIterations;
    orbx_voc_train_summary summary;
    orbx_voc_trainer *trainer = 0;
    if (orbx_voc_trainer_create(orbx_shim::Device(), k, L, (int)total, (int)counts.size(), &trainer) != ORBX_OK) { orbx_shim::Fail("ORBVocabulary::create"); return; }
    std::vector<int32_t> parent;
    std::vector<uint8_t> leaf, desc;
    std::vector<double> weights;
    bool ok = orbx_voc_trainer_add(trainer, bytes.data(), counts.data(), (int)counts.size()) == ORBX_OK && orbx_voc_train(trainer, &params, &summary) == ORBX_OK;
    if (ok) {
        const size_t n = (size_t)summary.num_nodes;
        parent.resize(n); leaf.resize(n); desc.resize(n * 32); weights.resize(n);
        ok = orbx_voc_trainer_result(trainer, parent.data(), leaf.data(), desc.data(), weights.data(), 0, summary.num_nodes) == ORBX_OK;
    }
    if (!ok) orbx_shim::Fail("ORBVocabulary::create");
    orbx_voc_trainer_destroy(trainer);
    if (!ok) return;

    mnUnconverged = summary.unconverged_nodes;
    m_nodes.resize((size_t)summary.num_nodes);
    for (int id = 1; id < summary.num_nodes; id++) {
        Node &nd = m_nodes[(size_t)id];
        nd.id = (DBoW2::NodeId)id;
        nd.parent = (DBoW2::NodeId)parent[(size_t)id];
        nd.weight = weights[(size_t)id];
        nd.descriptor = cv::Mat(1, 32, CV_8U);
        memcpy(nd.descriptor.ptr<unsigned char>(), &desc[(size_t)id * 32], 32);
        m_nodes[(size_t)parent[(size_t)id]].children.push_back((DBoW2::NodeId)id);      // ascending ids: the order HKmeansStep pushes them in
    }
    m_words.reserve((size_t)summary.num_words);
    for (int id = 1; id < summary.num_nodes; id++) {      // createWords: the leaves in node-id order
        if (!leaf[(size_t)id]) continue;
        m_nodes[(size_t)id].word_id = (DBoW2::WordId)m_words.size();
        m_words.push_back(&m_nodes[(size_t)id]);
    }
}
}  // namespace ORB_SLAM2
