// shim/Initializer_hip.h -- Initializer::Initialize in one device call (shim/Initializer_hip.cc; INTEGRATION.md, "Monocular initialisation").
#ifndef ORBX_SHIM_INITIALIZER_HIP_H
#define ORBX_SHIM_INITIALIZER_HIP_H

// Initializer_hip.cc DEFINES bool ORB_SLAM2::Initializer::Initialize(const Frame &, const vector<int> &, cv::Mat &, cv::Mat &,
// vector<cv::Point3f> &, vector<bool> &) of the reference's unmodified include/Initializer.h: a build that links it leaves that one
// function out of src/Initializer.cc.  Calls served so far (every thread):
extern "C" unsigned long orbx_shim_initialize_calls(void);

#endif
