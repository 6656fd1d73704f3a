"""orb-slam2_amd — MI355X-native ORB front end + Hamming matchers for ORB-SLAM2.

Host-side mirror (Python, ctypes) of the reference's operator interface for the hot path,
sitting directly on the C ABI of liborbx.so (include/orbx.h):

  ORBextractor          <- reference include/ORBextractor.h:58-139
  ORBmatcher            <- reference include/ORBmatcher.h:41-103 (the three north-star searches)
  ComputeStereoMatches  <- reference src/Frame.cc:577-751
  KeyFrameDatabase      <- reference include/KeyFrameDatabase.h:42-70 (relocalisation and loop candidate queries)
  ORBextractor.extract_rgbd / rgbd_depth_batch_device <- reference src/Frame.cc:145-154, :754-774 (RGB-D frames)
  pose_optimize / DeviceFrame.pose_optimize <- reference src/Optimizer.cc:286-513 (motion-only pose optimisation)
  triangulate_pairs / frame_triangulate <- reference src/LocalMapping.cc:327-511 (CreateNewMapPoints' triangulation)
  sim3_hypotheses / Sim3Ransac <- reference src/Sim3Solver.cc:117-433 (LoopClosing::ComputeSim3's RANSAC)
  sim3_optimize / sim3_optimize_batch <- reference src/Optimizer.cc:1164-1365 (Optimizer::OptimizeSim3)
  pnp_hypotheses / PnPRansac <- reference src/PnPsolver.cc:128-961 (Tracking::Relocalization's EPnP RANSAC)
  local_bundle_adjustment <- reference src/Optimizer.cc:528-862 (Optimizer::LocalBundleAdjustment, LocalMapping's optimisation)
  bundle_adjustment <- reference src/Optimizer.cc:48-281 (Optimizer::BundleAdjustment, the global bundle adjustment)
  optimize_essential_graph <- reference src/Optimizer.cc:885-1153 (Optimizer::OptimizeEssentialGraph, LoopClosing::CorrectLoop)
  MapGraph <- reference src/LocalMapping.cc:704-775, src/KeyFrame.cc:303-338, src/Tracking.cc:1515-1538 (KeyFrameCulling and the covisibility votes)
  MapGraph.refresh_points <- reference src/MapPoint.cc:266-340, :371-420 (ComputeDistinctiveDescriptors, UpdateNormalAndDepth)
  mono_init_hypotheses / mono_init_reconstruct / Initializer <- reference src/Initializer.cc:37-1026 (Tracking::MonocularInitialization)

There is NO CPU fallback: importing works without a GPU (so that the ABI can be inspected), but
every compute call raises OrbxError unless liborbx.so is built and a gfx950 device is present.
The directory name contains a '-', so load it with importlib (see tests/conftest.py: load_pkg()).
"""
from . import orbx, streams
from .orbx import (OrbxError, KP_DTYPE, lib, lib_path, ORBextractor, ORBmatcher, ComputeStereoMatches,
                   FeatSet, make_featset, STAGES, BowDatabase, DeviceKeyFrame, DeviceFrame, MapPoints, MapGraph, BowFrames, KeyFrameDatabase, ORBVocabulary, ComputeDistinctiveDescriptors, Rectifier, UndistortKeyPoints,
                   RGBDParams, depth_map_factor, rgbd_depth_batch_device, DEPTH_U16, DEPTH_F32, pose_optimize, pose_optimize_batch,
                   triangulate_pairs, frame_set_depth, frame_triangulate, sim3_hypotheses, sim3_hypotheses_batch, sim3_max_error, Sim3Ransac,
                   sim3_optimize, sim3_optimize_batch, sim3opt_camera_points, pnp_hypotheses, pnp_hypotheses_batch, PnPRansac,
                   mono_init_hypotheses, mono_init_reconstruct, mono_init_initialize, mono_init_draw_sets, DUtilsRandom, Initializer,
                   local_bundle_adjustment, bundle_adjustment, optimize_essential_graph, RefreshResult, REFRESH_GEOM, REFRESH_DESC)

__all__ = ["OrbxError", "KP_DTYPE", "lib", "lib_path", "ORBextractor", "ORBmatcher", "ComputeStereoMatches",
           "FeatSet", "make_featset", "STAGES", "BowDatabase", "DeviceKeyFrame", "DeviceFrame", "MapPoints", "MapGraph", "BowFrames", "KeyFrameDatabase", "ORBVocabulary", "ComputeDistinctiveDescriptors", "Rectifier", "UndistortKeyPoints",
           "RGBDParams", "depth_map_factor", "rgbd_depth_batch_device", "DEPTH_U16", "DEPTH_F32", "pose_optimize", "pose_optimize_batch",
           "triangulate_pairs", "frame_set_depth", "frame_triangulate", "sim3_hypotheses", "sim3_hypotheses_batch", "sim3_max_error", "Sim3Ransac",
           "sim3_optimize", "sim3_optimize_batch", "sim3opt_camera_points", "pnp_hypotheses", "pnp_hypotheses_batch", "PnPRansac",
           "mono_init_hypotheses", "mono_init_reconstruct", "mono_init_initialize", "mono_init_draw_sets", "DUtilsRandom", "Initializer",
           "local_bundle_adjustment", "bundle_adjustment", "optimize_essential_graph", "RefreshResult", "REFRESH_GEOM", "REFRESH_DESC"]
