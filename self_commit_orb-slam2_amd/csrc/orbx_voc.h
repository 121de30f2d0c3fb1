// orbx_voc.h -- the device form of a DBoW2 vocabulary tree, shared by the modules that build one (orbx_bow.hip: orbx_vocabulary_create from flat
// arrays; orbx_voc_text.hip: orbx_vocabulary_load_text from the text file) and by the descent that reads it (orbx_bow.hip).
//
//   nodes[i]        childStart / childCount: node i's children are childList[childStart .. childStart + childCount), in ASCENDING node id (the order
//                   loadFromTextFile pushes them in, reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1385-1392); word >= 0: a leaf and its word
//                   id - the leaves counted in node-id order (:1408-1415); the root is never a leaf
//   childDesc       the 32 descriptor bytes of childList[c] at uint4 2c, 2c + 1: the children of a node are contiguous for the descent
//   nodeWeight[i]   the weight of node i (leaves: the word weight)
#ifndef ORBX_VOC_H
#define ORBX_VOC_H

#include "orbx_handle.h"

struct VocNode { int32_t childStart, childCount, word, pad; };   // word >= 0: leaf

struct orbx_vocabulary : OrbxHandle {      // (the stream: host-array form only; the device form runs on the extractor's stream)
    int k = 0, L = 0, numNodes = 0, numWords = 0;
    OrbxOwnedBuf<VocNode> nodes;
    OrbxOwnedBuf<int32_t> childList;
    OrbxOwnedBuf<uint4> childDesc;
    OrbxOwnedBuf<double> nodeWeight;
    // results, double buffered in lockstep with the extractor's result buffers
    OrbxOwnedBuf<int32_t> word[2], node[2];
    OrbxOwnedBuf<double> weight[2];
    int cur = 0, lastBatch = 0, lastCap = 0;
    OrbxCallBox box;   // host-array form: descriptors in, word / node / weight out through mapped pinned memory
    OrbxOwnedBuf<int32_t> hostWord, hostNode;   // host-array _sorted form: the device copy k_bow_ranks reads - its own, never the device form's word[] / node[] (a
                                              // host call between two device calls must leave the last batch's results, and the pointers handed out, alone)
};

#endif
