// shim/ORBVocabulary_hip.cc -- TemplatedVocabulary::create(training_features, k, L, weighting, scoring)
// (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:604-616 over :557-587) through orbx_voc_train, and TemplatedVocabulary::loadFromTextFile
// (:1338-1420) through orbx_vocabulary_load_text.
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
#include <string>
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

ORBVocabulary_hip::~ORBVocabulary_hip()
{
    if (mpDevice) orbx_vocabulary_destroy(mpDevice);
}

// :1338-1420 with the parse and the tree on the device.  What stays on the host: m_nodes / m_words from the flat arrays (1.1 M cv::Mat at the
// shape of ORBvoc.txt).  The reference's extra node behind a final newline is not made (include/orbx.h); a malformed file, which the reference
// reads into zeros and stale values, is refused: false, vocabulary empty, counted and printed by orbx_shim::Fail.
bool ORBVocabulary_hip::loadFromTextFile(const std::string &filename)
{
    m_words.clear();
    m_nodes.clear();
    if (mpDevice) { orbx_vocabulary_destroy(mpDevice); mpDevice = 0; }

    orbx_voc_text_info info;
    orbx_vocabulary *voc = 0;
    if (orbx_vocabulary_load_text(orbx_shim::Device(), filename.c_str(), &voc, &info) != ORBX_OK) { orbx_shim::Fail("ORBVocabulary::loadFromTextFile"); return false; }
    const size_t n = (size_t)info.num_nodes;
    std::vector<int32_t> parent(n);
    std::vector<uint8_t> leaf(n), desc(n * 32);
    std::vector<double> weights(n);
    if (orbx_vocabulary_tree(voc, 0, 0, 0, parent.data(), leaf.data(), desc.data(), weights.data()) != ORBX_OK) {
        orbx_shim::Fail("ORBVocabulary::loadFromTextFile");
        orbx_vocabulary_destroy(voc);
        return false;
    }
    m_k = info.k;
    m_L = info.L;
    m_scoring = (DBoW2::ScoringType)info.scoring;
    m_weighting = (DBoW2::WeightingType)info.weighting;
    createScoringObject();

    m_nodes.resize(n);
    m_nodes[0].id = 0;
    m_words.reserve((size_t)info.num_words);
    for (size_t id = 1; id < n; id++) {      // in id order, as the lines come: children in ascending id (:1392), words in node-id order (:1408-1415)
        Node &nd = m_nodes[id];
        nd.id = (DBoW2::NodeId)id;
        nd.parent = (DBoW2::NodeId)parent[id];
        m_nodes[(size_t)parent[id]].children.push_back((DBoW2::NodeId)id);
        nd.descriptor = cv::Mat(1, 32, CV_8U);
        memcpy(nd.descriptor.ptr<unsigned char>(), &desc[id * 32], 32);
        nd.weight = weights[id];
        if (leaf[id]) {
            nd.word_id = (DBoW2::WordId)m_words.size();
            m_words.push_back(&nd);
        } else
            nd.children.reserve((size_t)m_k);
    }
    mpDevice = voc;
    return true;
}
}  // namespace ORB_SLAM2
