"""ctypes binding of liborbx.so + mirror classes named after the reference's C++ interface."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("ORBX_SO") or os.path.join(_HERE, "liborbx.so")  # ORBX_SO: diagnostic builds only

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])  # == cv::KeyPoint, 28 B
STAGES = ("resize", "fast", "tree", "desc", "stereo", "stereo_cut")


class OrbxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"orbx error {code}: {msg}")
        self.code = code


class FeatSet(C.Structure):
    """orbx_featset (include/orbx.h)"""
    _fields_ = [("n", C.c_int), ("desc", C.c_void_p), ("nnodes", C.c_int), ("node_id", C.c_void_p),
                ("node_off", C.c_void_p), ("feat", C.c_void_p), ("flag", C.c_void_p), ("angle", C.c_void_p),
                ("x", C.c_void_p), ("y", C.c_void_p), ("octave", C.c_void_p), ("u_right", C.c_void_p)]


class FrameFeats(C.Structure):
    """orbx_frame_feats (include/orbx.h)"""
    _fields_ = [("n", C.c_int), ("x", C.c_void_p), ("y", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p),
                ("u_right", C.c_void_p), ("desc", C.c_void_p), ("occupied", C.c_void_p),
                ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float)]


DEPTH_U16, DEPTH_F32 = 0, 1   # ORBX_DEPTH_*: CV_16U (TUM PNG depth) / CV_32F


class RGBDParamsStruct(C.Structure):
    """orbx_rgbd_params (include/orbx.h)"""
    _fields_ = [("depth_type", C.c_int), ("depth_scale", C.c_float), ("bf", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("dist_coef", C.c_float * 5), ("ndist", C.c_int)]


def depth_map_factor(DepthMapFactor):
    """Tracking::mDepthMapFactor from the settings value (reference src/Tracking.cc:147-151), in float32 as the reference holds it:
    1 when |DepthMapFactor| < 1e-5, else 1.0f / DepthMapFactor"""
    f = np.float32(DepthMapFactor)
    if abs(float(f)) < 1e-5:
        return np.float32(1)
    return np.float32(np.float32(1) / f)


class RGBDParams:
    """camera and depth settings of an RGB-D frame (Examples/RGB-D/TUM*.yaml: Camera.fx/fy/cx/cy, k1 k2 p1 p2 [k3], Camera.bf,
    DepthMapFactor).  depth_scale defaults to depth_map_factor(DepthMapFactor); pass it to give Tracking::mDepthMapFactor directly."""

    def __init__(self, fx, fy, cx, cy, dist_coef, bf, DepthMapFactor=None, depth_scale=None):
        if (DepthMapFactor is None) == (depth_scale is None):
            raise OrbxError(-1, "give exactly one of DepthMapFactor and depth_scale")
        self.fx, self.fy, self.cx, self.cy = (np.float32(v) for v in (fx, fy, cx, cy))
        self.dist_coef = np.ascontiguousarray(dist_coef, np.float32).reshape(-1)
        self.bf = np.float32(bf)
        self.depth_scale = depth_map_factor(DepthMapFactor) if depth_scale is None else np.float32(depth_scale)

    @classmethod
    def from_settings(cls, s):
        """from a dict of the yaml keys (tests/golden/reference_settings_rgbd.json: one camera entry)"""
        d = [s["Camera.k1"], s["Camera.k2"], s["Camera.p1"], s["Camera.p2"]] + ([s["Camera.k3"]] if "Camera.k3" in s else [])
        return cls(s["Camera.fx"], s["Camera.fy"], s["Camera.cx"], s["Camera.cy"], d, s["Camera.bf"], DepthMapFactor=s["DepthMapFactor"])

    def struct(self, depth_type):
        p = RGBDParamsStruct()
        p.depth_type = int(depth_type); p.depth_scale = float(self.depth_scale); p.bf = float(self.bf)
        p.fx, p.fy, p.cx, p.cy = float(self.fx), float(self.fy), float(self.cx), float(self.cy)
        for k, v in enumerate(self.dist_coef[:5]):
            p.dist_coef[k] = float(v)
        p.ndist = len(self.dist_coef)
        return p


def _depth_type(depth):
    if depth.dtype == np.uint16:
        return DEPTH_U16
    if depth.dtype == np.float32:
        return DEPTH_F32
    raise OrbxError(-1, "depth must be uint16 (CV_16U) or float32 (CV_32F)")


def _rgbd_image(image):
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] not in (3, 4)):
        raise OrbxError(-1, "image must be H x W uint8 or H x W x 3|4 uint8")
    if image.strides[-1] != 1 or (image.ndim == 3 and image.strides[1] != image.shape[2]):
        image = np.ascontiguousarray(image)
    return image, (1 if image.ndim == 2 else image.shape[2])


def _rgbd_depth(depth):
    depth = np.asarray(depth)
    if depth.ndim != 2 or depth.strides[1] != depth.itemsize:
        depth = np.ascontiguousarray(depth)
    return depth


class ProjPoints(C.Structure):
    """orbx_proj_points (include/orbx.h)"""
    _fields_ = [("n", C.c_int), ("u", C.c_void_p), ("v", C.c_void_p), ("aux", C.c_void_p), ("level", C.c_void_p),
                ("angle", C.c_void_p), ("view_cos", C.c_void_p), ("desc", C.c_void_p), ("valid", C.c_void_p), ("has_obs", C.c_void_p)]


class WindowJob(C.Structure):
    """orbx_window_job (include/orbx.h)"""
    _fields_ = [("kf", C.c_void_p), ("pts", C.POINTER(ProjPoints)), ("scale_factors", C.c_void_p), ("inv_sigma2", C.c_void_p),
                ("nlevels", C.c_int), ("th", C.c_float), ("chi2", C.c_int), ("max_dist", C.c_int), ("best_idx", C.c_void_p),
                ("best_dist", C.c_void_p), ("nfound", C.c_int)]


class PoseObs(C.Structure):
    """orbx_pose_obs (include/orbx.h)"""
    _fields_ = [("n", C.c_int), ("x", C.c_void_p), ("y", C.c_void_p), ("u_right", C.c_void_p), ("inv_sigma2", C.c_void_p),
                ("Xw", C.c_void_p), ("has_point", C.c_void_p)]


class PoseReport(C.Structure):
    """orbx_pose_report (include/orbx.h)"""
    _fields_ = [("n_corr", C.c_int), ("rounds", C.c_int), ("n_bad", C.c_int * 4), ("iterations", C.c_int * 4),
                ("chi2", C.c_double * 4), ("pose", C.c_double * 12)]


class LbaProblem(C.Structure):
    """orbx_lba_problem (include/orbx.h)"""
    _fields_ = [("n_kf", C.c_int), ("Tcw", C.c_void_p), ("cam", C.c_void_p), ("fixed", C.c_void_p), ("n_points", C.c_int), ("Xw", C.c_void_p),
                ("n_edges", C.c_int), ("edge_kf", C.c_void_p), ("edge_point", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p),
                ("u_right", C.c_void_p), ("inv_sigma2", C.c_void_p)]


class LbaOptions(C.Structure):
    """orbx_lba_options (include/orbx.h)"""
    _fields_ = [("stop", C.c_void_p), ("debug_stop_at_trial", C.c_int)]


class LbaReport(C.Structure):
    """orbx_lba_report (include/orbx.h)"""
    _fields_ = [("stopped", C.c_int), ("iterations", C.c_int * 2), ("trials", C.c_int * 2), ("n_level1", C.c_int), ("n_erase", C.c_int),
                ("n_active_kf", C.c_int * 2), ("n_active_points", C.c_int * 2), ("chi2", C.c_double * 2), ("lambda_", C.c_double * 2)]


class BaOptions(C.Structure):
    """orbx_ba_options (include/orbx.h)"""
    _fields_ = [("stop", C.c_void_p), ("debug_stop_at_trial", C.c_int), ("iterations", C.c_int), ("robust", C.c_int)]


class BaReport(C.Structure):
    """orbx_ba_report (include/orbx.h)"""
    _fields_ = [("stopped", C.c_int), ("iterations", C.c_int), ("trials", C.c_int), ("n_active_kf", C.c_int), ("n_active_points", C.c_int),
                ("chi2", C.c_double), ("lambda_", C.c_double), ("lambda_init", C.c_double)]


class EgProblem(C.Structure):
    """orbx_eg_problem (include/orbx.h)"""
    _fields_ = [("n_kf", C.c_int), ("Tcw", C.c_void_p), ("fixed", C.c_void_p), ("corrected", C.c_void_p), ("noncorrected", C.c_void_p),
                ("n_corrected", C.c_int), ("n_noncorrected", C.c_int), ("S_corrected", C.c_void_p), ("S_noncorrected", C.c_void_p),
                ("n_edges", C.c_int), ("edge_i", C.c_void_p), ("edge_j", C.c_void_p), ("edge_kind", C.c_void_p),
                ("n_points", C.c_int), ("Xw", C.c_void_p), ("point_ref", C.c_void_p), ("fix_scale", C.c_int)]


class EgOptions(C.Structure):
    """orbx_eg_options (include/orbx.h)"""
    _fields_ = [("iterations", C.c_int)]


class EgOptions2(C.Structure):
    """orbx_eg_options2 (include/orbx.h)"""
    _fields_ = [("iterations", C.c_int), ("solver", C.c_int)]


EG_SOLVER_DENSE, EG_SOLVER_ENVELOPE, EG_SOLVER_AUTO = 0, 1, 2
EG_MAX_ENVELOPE = 1 << 27


class EgReport(C.Structure):
    """orbx_eg_report (include/orbx.h)"""
    _fields_ = [("iterations", C.c_int), ("trials", C.c_int), ("n_free", C.c_int), ("n_solve_failed", C.c_int),
                ("chi2_start", C.c_double), ("chi2", C.c_double), ("lambda_", C.c_double)]


class EgStages(C.Structure):
    """orbx_eg_stages (include/orbx.h)"""
    _fields_ = [(k, C.c_void_p) for k in ("vS", "meas", "xf", "rec", "echi", "Hd", "bv", "n_pairs", "pair", "Off", "status_lin", "err", "S", "y",
                                          "solve_ok", "x", "trial", "sc", "echi_trial", "status_trial")]


class PoseJob(C.Structure):
    """orbx_pose_job (include/orbx.h)"""
    _fields_ = [("obs", C.POINTER(PoseObs)), ("cam", C.c_void_p), ("Tcw", C.c_void_p), ("Tcw_out", C.c_void_p),
                ("outlier", C.c_void_p), ("n_inliers", C.c_int), ("report", C.POINTER(PoseReport))]


class TriView(C.Structure):
    """orbx_tri_view (include/orbx.h)"""
    _fields_ = [("Tcw", C.c_float * 12), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("invfx", C.c_float), ("invfy", C.c_float), ("mb", C.c_float), ("mbf", C.c_float)]


class TriFeats(C.Structure):
    """orbx_tri_feats (include/orbx.h)"""
    _fields_ = [("n", C.c_int), ("x", C.c_void_p), ("y", C.c_void_p), ("octave", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p),
                ("raw_x", C.c_void_p), ("raw_y", C.c_void_p)]


class Sim3Job(C.Structure):
    """orbx_sim3_job (include/orbx.h)"""
    _fields_ = [("n", C.c_int), ("X1", C.c_void_p), ("X2", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p),
                ("K1", C.c_float * 4), ("K2", C.c_float * 4), ("fix_scale", C.c_int), ("n_hyp", C.c_int), ("samples", C.c_void_p),
                ("n_inliers", C.c_void_p), ("srt", C.c_void_p), ("inlier_bits", C.c_void_p)]


class PnpJob(C.Structure):
    """orbx_pnp_job (include/orbx.h)"""
    _fields_ = [("n", C.c_int), ("P3Dw", C.c_void_p), ("P2D", C.c_void_p), ("max_err", C.c_void_p), ("K", C.c_double * 4),
                ("min_inliers", C.c_int), ("n_hyp", C.c_int), ("samples", C.c_void_p),
                ("n_inliers", C.c_void_p), ("Rt", C.c_void_p), ("inlier_bits", C.c_void_p),
                ("n_refined", C.c_void_p), ("Rt_refined", C.c_void_p), ("refined_bits", C.c_void_p)]


class MonoInitJob(C.Structure):
    """orbx_mono_init_job (include/orbx.h)"""
    _fields_ = [("n1", C.c_int), ("n2", C.c_int), ("xy1", C.c_void_p), ("xy2", C.c_void_p), ("n", C.c_int), ("matches", C.c_void_p),
                ("sigma", C.c_float), ("K", C.c_float * 4), ("min_parallax", C.c_float), ("min_triangulated", C.c_int),
                ("n_hyp", C.c_int), ("samples", C.c_void_p),
                ("score_h", C.c_void_p), ("score_f", C.c_void_p), ("H21", C.c_void_p), ("F21", C.c_void_p),
                ("bits_h", C.c_void_p), ("bits_f", C.c_void_p)]


class MonoInitRecon(C.Structure):
    """orbx_mono_init_recon (include/orbx.h)"""
    _fields_ = [("ok", C.c_int), ("winner", C.c_int), ("n_good", C.c_int32 * 8), ("cos_parallax", C.c_float * 8),
                ("R", C.c_float * 72), ("t", C.c_float * 24), ("P3D", C.c_void_p), ("triangulated", C.c_void_p)]


class MonoInitResult(C.Structure):
    """orbx_mono_init_result (include/orbx.h)"""
    _fields_ = [("ok", C.c_int), ("model", C.c_int), ("best_h", C.c_int), ("best_f", C.c_int), ("SH", C.c_float), ("SF", C.c_float),
                ("M", C.c_float * 9), ("R21", C.c_float * 9), ("t21", C.c_float * 3), ("parallax", C.c_float), ("winner", C.c_int),
                ("n_good", C.c_int32 * 8), ("cos_parallax", C.c_float * 8), ("P3D", C.c_void_p), ("triangulated", C.c_void_p)]


class Sim3OptObs(C.Structure):
    """orbx_sim3opt_obs (include/orbx.h)"""
    _fields_ = [("n", C.c_int), ("has_pair", C.c_void_p), ("P1c", C.c_void_p), ("P2c", C.c_void_p), ("x1", C.c_void_p), ("y1", C.c_void_p),
                ("inv_sigma2_1", C.c_void_p), ("x2", C.c_void_p), ("y2", C.c_void_p), ("inv_sigma2_2", C.c_void_p)]


class Sim3OptReport(C.Structure):
    """orbx_sim3opt_report (include/orbx.h)"""
    _fields_ = [("n_corr", C.c_int), ("rounds", C.c_int), ("n_bad", C.c_int), ("more_iterations", C.c_int), ("iterations", C.c_int * 2),
                ("chi2", C.c_double * 2), ("S12", C.c_double * 8)]


class Sim3OptJob(C.Structure):
    """orbx_sim3opt_job (include/orbx.h)"""
    _fields_ = [("obs", C.POINTER(Sim3OptObs)), ("cam1", C.c_void_p), ("cam2", C.c_void_p), ("S12", C.c_void_p), ("th2", C.c_float),
                ("fix_scale", C.c_int), ("S12_out", C.c_void_p), ("inlier", C.c_void_p), ("n_inliers", C.c_int),
                ("report", C.POINTER(Sim3OptReport))]


class RefreshJob(C.Structure):
    """orbx_refresh_job (include/orbx.h)"""
    _fields_ = [("what", C.c_int), ("n", C.c_int), ("point", C.c_void_p), ("table_slot", C.c_void_p), ("pos", C.c_void_p),
                ("ref_kf", C.c_void_p), ("nk", C.c_int), ("kf_slot", C.c_void_p), ("kf_centre", C.c_void_p), ("kf_bad", C.c_void_p),
                ("kf_frame", C.POINTER(C.c_void_p)), ("scale_factors", C.c_void_p), ("nlevels", C.c_int)]


REFRESH_GEOM, REFRESH_DESC = 1, 2


class RefreshResult:
    """what MapGraph.refresh_points hands back: status[n] (bit 0 geometry, bit 1 descriptor), geom[n][8] = X Y Z mfMinDistance nx ny nz
    mfMaxDistance, best_kf[n], best_idx[n], desc[n][32]; a row whose status bit is clear is as it was before the call"""

    def __init__(self, n, fill=0):
        self.status = np.full(n, fill, np.uint8)
        self.geom = np.full((n, 32), fill, np.uint8).view(np.float32)      # [n][8]; fill is a byte pattern
        self.best_kf = np.full((n, 4), fill, np.uint8).view(np.int32).reshape(n)
        self.best_idx = self.best_kf.copy()
        self.desc = np.full((n, 32), fill, np.uint8)


_lib = None


def lib_path():
    return _SO


def lib():
    """Load liborbx.so; fail loudly if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise OrbxError(-4, f"{_SO} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(_SO)
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    L.orbx_last_error.restype = C.c_char_p
    L.orbx_device_count.restype = i
    L.orbx_device_identity.argtypes = [i, C.c_char_p, i]
    L.orbx_extractor_create.argtypes = [C.POINTER(vp), i, f, i, i, i, i, i, i, i]
    L.orbx_extractor_set_cv_profile.argtypes = [vp, i]
    L.orbx_extractor_set_pyramid_group_limit.argtypes = [vp, i]
    L.orbx_gaussian_taps.argtypes = [i, vp]
    L.orbx_desc_rowpass_matrix.argtypes = [i, vp, ip]
    L.orbx_extractor_destroy.argtypes = [vp]
    L.orbx_extractor_destroy.restype = None
    L.orbx_get_levels.argtypes = [vp]
    L.orbx_get_scale_factor.argtypes = [vp]
    L.orbx_get_scale_factor.restype = f
    L.orbx_get_scale_tables.argtypes = [vp, vp, vp, vp, vp]
    L.orbx_get_features_per_level.argtypes = [vp, vp]
    L.orbx_max_keypoints.argtypes = [vp, i, i]
    L.orbx_extract.argtypes = [vp, vp, i, i, sz, vp, vp, i, ip]
    L.orbx_extract_stereo.argtypes = [vp, vp, vp, i, i, sz, f, f, vp, vp, i, vp, vp, vp]
    L.orbx_extract_stereo_submit.argtypes = [vp, vp, vp, i, i, sz, f, f, ip]
    L.orbx_extract_stereo_wait.argtypes = [vp, i, vp, vp, i, vp, vp, vp]
    L.orbx_extract_submit.argtypes = [vp, vp, i, i, sz, ip]
    L.orbx_pipeline_warm.argtypes = [vp, i, i]
    L.orbx_extract_wait.argtypes = [vp, i, vp, vp, i, vp]
    L.orbx_pinned_alloc.argtypes = [sz]; L.orbx_pinned_alloc.restype = vp
    L.orbx_pinned_free.argtypes = [vp]; L.orbx_pinned_free.restype = None
    L.orbx_extract_color.argtypes = [vp, vp, i, i, sz, i, i, vp, vp, i, ip, vp, sz]
    L.orbx_extract_batch.argtypes = [vp, vp, i, i, i, sz, vp, vp, i, vp]
    L.orbx_extract_batch_device.argtypes = [vp, vp, sz, sz, i, i, i, vp, vp, i, vp, vp]
    L.orbx_sync.argtypes = [vp, vp]
    L.orbx_pyramid_level.argtypes = [vp, i, i, vp, sz, ip, ip]
    L.orbx_stereo_match.argtypes = [vp, vp, vp, vp, i, vp, vp, i, f, f, vp, vp]
    L.orbx_stereo_match_batch_device.argtypes = [vp, i, vp, i, i, vp, vp, vp, vp, vp, vp, i, f, f, vp, vp, i, vp]
    L.orbx_stereo_row_table_available.argtypes = [vp, vp, i, i, i]
    L.orbx_hamming.argtypes = [vp, vp]
    FS = C.POINTER(FeatSet)
    L.orbx_search_by_bow_kf_f.argtypes = [i, FS, FS, f, i, vp, ip]
    L.orbx_search_by_bow_kf_f_batch.argtypes = [i, FS, i, FS, f, i, vp, vp]
    L.orbx_search_by_bow_kf_kf.argtypes = [i, FS, FS, f, i, vp, ip]
    L.orbx_search_for_triangulation.argtypes = [i, FS, FS, vp, f, f, vp, vp, i, i, i, vp, i, ip]
    L.orbx_search_by_bow_kf_kf_batch.argtypes = [i, FS, FS, i, f, i, vp, vp]
    L.orbx_search_for_triangulation_batch.argtypes = [i, FS, FS, i, vp, vp, vp, vp, i, i, i, vp, i, vp]
    L.orbx_kf_create.argtypes = [i, FS, C.POINTER(vp)]
    L.orbx_kf_destroy.argtypes = [vp]; L.orbx_kf_destroy.restype = None
    L.orbx_kf_size.argtypes = [vp]
    L.orbx_kf_search_by_bow_kf_f.argtypes = [vp, vp, vp, f, i, vp, ip]
    L.orbx_kf_search_by_bow_kf_kf.argtypes = [vp, vp, vp, vp, i, f, i, vp, vp]
    L.orbx_kf_search_by_bow_kfs_f.argtypes = [vp, vp, i, FS, f, i, vp, vp]
    L.orbx_kf_search_for_triangulation.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, i, i, i, vp, i, vp]
    L.orbx_bowdb_create.argtypes = [i, FS, i, C.POINTER(vp)]
    L.orbx_bowdb_search.argtypes = [vp, FS, f, i, vp, vp]
    L.orbx_bowdb_size.argtypes = [vp]
    L.orbx_bowdb_destroy.argtypes = [vp]
    L.orbx_bowdb_destroy.restype = None
    L.orbx_vocab_create.argtypes = [i, i, i, i, vp, vp, vp, vp, C.POINTER(vp)]
    L.orbx_vocab_load_text.argtypes = [i, C.c_char_p, C.POINTER(vp)]
    L.orbx_vocab_info.argtypes = [vp, ip, ip, ip, ip]
    L.orbx_vocab_destroy.argtypes = [vp]
    L.orbx_vocab_destroy.restype = None
    L.orbx_bow_transform.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp, ip, vp, vp, vp, ip]
    L.orbx_search_by_projection_last_frame.argtypes = [i, C.POINTER(FrameFeats), C.POINTER(ProjPoints), vp, i, f, i, f, i, vp, ip]
    L.orbx_search_by_projection_map_points.argtypes = [i, C.POINTER(FrameFeats), C.POINTER(ProjPoints), vp, i, f, f, vp, ip]
    L.orbx_search_by_projection_keyframe.argtypes = [i, C.POINTER(FrameFeats), C.POINTER(ProjPoints), vp, i, f, i, i, vp, ip]
    L.orbx_search_by_projection_sim3.argtypes = [i, C.POINTER(FrameFeats), C.POINTER(ProjPoints), vp, i, f, vp, ip]
    L.orbx_window_best.argtypes = [i, C.POINTER(FrameFeats), C.POINTER(ProjPoints), vp, vp, i, f, i, i, vp, vp, ip]
    L.orbx_frame_create.argtypes = [i, C.POINTER(FrameFeats), C.POINTER(vp)]
    L.orbx_frame_create_from_extraction.argtypes = [i, vp, vp, vp, i, i, vp, vp, vp, i, f, f, f, f, vp, C.POINTER(vp)]
    L.orbx_frame_size.argtypes = [vp]
    L.orbx_frame_read.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.orbx_frame_destroy.argtypes = [vp]; L.orbx_frame_destroy.restype = None
    L.orbx_frame_search_by_projection_last_frame.argtypes = [vp, vp, C.POINTER(ProjPoints), vp, i, f, i, f, i, vp, ip]
    L.orbx_frame_search_by_projection_map_points.argtypes = [vp, vp, C.POINTER(ProjPoints), vp, i, f, f, vp, ip]
    L.orbx_frame_search_by_projection_keyframe.argtypes = [vp, vp, C.POINTER(ProjPoints), vp, i, f, i, i, vp, ip]
    L.orbx_frame_window_best.argtypes = [vp, C.POINTER(ProjPoints), vp, vp, i, f, i, i, vp, vp, ip]
    L.orbx_frame_window_best_batch.argtypes = [C.POINTER(WindowJob), i]
    L.orbx_frame_search_by_projection_sim3.argtypes = [vp, vp, C.POINTER(ProjPoints), vp, i, f, vp, ip]
    L.orbx_frame_search_by_sim3.argtypes = [vp, vp, C.POINTER(ProjPoints), C.POINTER(ProjPoints), vp, vp, i, f, vp, ip]
    L.orbx_mappoints_create.argtypes = [i, i, C.POINTER(vp)]
    L.orbx_mappoints_destroy.argtypes = [vp]; L.orbx_mappoints_destroy.restype = None
    L.orbx_mappoints_capacity.argtypes = [vp]
    L.orbx_mappoints_set.argtypes = [vp, vp, i, vp, vp, vp]
    L.orbx_mappoints_read.argtypes = [vp, vp, i, vp, vp]
    L.orbx_mappoints_frustum.argtypes = [vp, vp, vp, i, vp, vp, f, f, i, vp, vp, vp, vp, vp, vp]
    L.orbx_mapgraph_create.argtypes = [i, i, i, i, i, C.POINTER(vp)]
    L.orbx_mapgraph_destroy.argtypes = [vp]; L.orbx_mapgraph_destroy.restype = None
    L.orbx_mapgraph_clear.argtypes = [vp]
    L.orbx_mapgraph_set_keyframe.argtypes = [vp, i, i, vp, vp, vp]
    L.orbx_mapgraph_set_matches.argtypes = [vp, i, vp, vp, i]
    L.orbx_mapgraph_add_observations.argtypes = [vp, vp, vp, vp, i]
    L.orbx_mapgraph_erase_observations.argtypes = [vp, vp, vp, i]
    L.orbx_mapgraph_erase_points.argtypes = [vp, vp, i]
    L.orbx_mapgraph_erase_keyframe.argtypes = [vp, i]
    L.orbx_mapgraph_keyframe_observations.argtypes = [vp, i]
    L.orbx_mapgraph_read_keyframe.argtypes = [vp, i, ip, vp, vp, vp, vp]
    L.orbx_mapgraph_read_points.argtypes = [vp, i, i, vp, vp, vp, vp, vp]
    L.orbx_mapgraph_vote.argtypes = [vp, vp, i, vp, vp, ip]
    L.orbx_mapgraph_covisibility.argtypes = [vp, i, vp, vp, ip]
    L.orbx_mapgraph_cull_keyframes.argtypes = [vp, vp, vp, i, i, vp, vp, vp, vp, i, ip]
    L.orbx_mapgraph_refresh_points.argtypes = [vp, vp, C.POINTER(RefreshJob), vp, vp, vp, vp, vp, vp]
    L.orbx_frame_search_local_points.argtypes = [vp, vp, vp, vp, vp, i, vp, vp, f, f, vp, i, f, f, vp, ip, vp]
    L.orbx_pose_optimize.argtypes = [i, C.POINTER(PoseObs), vp, vp, vp, vp, ip, C.POINTER(PoseReport)]
    L.orbx_pose_optimize_batch.argtypes = [i, C.POINTER(PoseJob), i]
    L.orbx_frame_pose_optimize.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, ip, C.POINTER(PoseReport)]
    L.orbx_local_bundle_adjustment.argtypes = [i, C.POINTER(LbaProblem), C.POINTER(LbaOptions), vp, vp, vp, vp, vp, C.POINTER(LbaReport)]
    L.orbx_debug_lba_profile.argtypes = [i, vp, vp]
    L.orbx_bundle_adjustment.argtypes = [i, C.POINTER(LbaProblem), C.POINTER(BaOptions), vp, vp, vp, vp, vp, C.POINTER(BaReport)]
    L.orbx_optimize_essential_graph.argtypes = [i, C.POINTER(EgProblem), C.POINTER(EgOptions), vp, vp, vp, vp, C.POINTER(EgReport)]
    L.orbx_optimize_essential_graph2.argtypes = [i, C.POINTER(EgProblem), C.POINTER(EgOptions2), vp, vp, vp, vp, C.POINTER(EgReport)]
    L.orbx_eg_envelope.argtypes = [C.POINTER(EgProblem), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.orbx_debug_eg_profile.argtypes = [i, vp, vp]
    L.orbx_debug_eg_stages.argtypes = [i, C.POINTER(EgProblem), C.c_double, vp, i, C.POINTER(EgStages)]
    L.orbx_debug_ldlt_solve.argtypes = [i, i, vp, vp, vp, i, C.POINTER(C.c_int)]
    L.orbx_debug_ldlt_solve_envelope.argtypes = [i, i, vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.orbx_debug_set_lba_solver.argtypes = [i]
    L.orbx_debug_ldlt_panel_width.argtypes = []
    L.orbx_triangulate_pairs.argtypes = [i, C.POINTER(TriFeats), C.POINTER(TriView), C.POINTER(C.POINTER(TriFeats)), C.POINTER(TriView), i, vp, i, vp,
                                         vp, vp, i, f, vp, vp, ip]
    L.orbx_frame_set_depth.argtypes = [vp, vp, vp, vp]
    L.orbx_frame_triangulate.argtypes = [vp, C.POINTER(TriView), C.POINTER(vp), C.POINTER(TriView), i, vp, i, vp, vp, vp, i, f, vp, vp, ip]
    L.orbx_sim3_hypotheses.argtypes = [i, C.POINTER(Sim3Job)]
    L.orbx_sim3_hypotheses_batch.argtypes = [i, C.POINTER(Sim3Job), i]
    L.orbx_pnp_hypotheses.argtypes = [i, C.POINTER(PnpJob)]
    L.orbx_pnp_hypotheses_batch.argtypes = [i, C.POINTER(PnpJob), i]
    L.orbx_mono_init_hypotheses.argtypes = [i, C.POINTER(MonoInitJob)]
    L.orbx_mono_init_reconstruct.argtypes = [i, C.POINTER(MonoInitJob), i, vp, vp, C.POINTER(MonoInitRecon)]
    L.orbx_mono_init_initialize.argtypes = [i, C.POINTER(MonoInitJob), C.POINTER(MonoInitResult)]
    L.orbx_sim3_optimize.argtypes = [i, C.POINTER(Sim3OptObs), vp, vp, vp, f, i, vp, vp, ip, C.POINTER(Sim3OptReport)]
    L.orbx_sim3_optimize_batch.argtypes = [i, C.POINTER(Sim3OptJob), i]
    L.orbx_bow_frames_create.argtypes = [i, i, i, C.POINTER(vp)]
    L.orbx_bow_frames_destroy.argtypes = [vp]; L.orbx_bow_frames_destroy.restype = None
    L.orbx_bow_transform_batch_device.argtypes = [vp, vp, vp, vp, vp, i, i, vp]
    L.orbx_bow_frames_read.argtypes = [vp, i, vp, vp, vp, ip, vp, vp, vp, ip]
    L.orbx_bowdb_search_batch_device.argtypes = [vp, vp, i, f, i, vp, vp, vp]
    L.orbx_bowdb_search_batch_device_compact.argtypes = [vp, vp, i, f, i, vp, i, vp, vp]
    L.orbx_bowdb_search_candidates_device.argtypes = [vp, vp, i, vp, i, vp, vp, i, f, i, vp, vp, vp]
    L.orbx_bowdb_search_candidates_device_compact.argtypes = [vp, vp, i, vp, i, vp, vp, i, f, i, vp, i, vp, vp]
    L.orbx_bowdb_create_live.argtypes = [i, i, i, i, C.POINTER(vp)]
    L.orbx_bowdb_add_from_frames.argtypes = [vp, i, vp, i, vp, vp]
    L.orbx_bowdb_add.argtypes = [vp, i, FS, vp]
    L.orbx_bowdb_erase.argtypes = [vp, i, vp]
    L.orbx_bowdb_set_flags.argtypes = [vp, vp, i, C.POINTER(vp), vp]
    L.orbx_bowdb_live_count.argtypes = [vp]
    L.orbx_bowdb_ids.argtypes = [vp, vp, i]
    L.orbx_bowdb_read_keyframe.argtypes = [vp, i, ip, ip, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbx_kfdb_create.argtypes = [i, i, C.POINTER(vp)]
    L.orbx_kfdb_destroy.argtypes = [vp]; L.orbx_kfdb_destroy.restype = None
    L.orbx_kfdb_size.argtypes = [vp]
    L.orbx_kfdb_next_id.argtypes = [vp]
    L.orbx_kfdb_clear.argtypes = [vp]
    L.orbx_kfdb_add.argtypes = [vp, vp, vp, i, ip]
    L.orbx_kfdb_add_from_frames.argtypes = [vp, vp, i, vp, ip]
    L.orbx_kfdb_erase.argtypes = [vp, i]
    L.orbx_kfdb_set_covisibility.argtypes = [vp, i, vp, i]
    L.orbx_kfdb_score.argtypes = [vp, vp, vp, i, vp, i, vp]
    L.orbx_kfdb_score_frame.argtypes = [vp, vp, i, vp, i, vp]
    L.orbx_kfdb_detect_relocalization.argtypes = [vp, vp, vp, i, vp, i, ip, vp, vp]
    L.orbx_kfdb_detect_relocalization_frame.argtypes = [vp, vp, i, vp, i, ip, vp, vp]
    L.orbx_kfdb_detect_loop.argtypes = [vp, vp, vp, i, vp, i, f, vp, i, ip, vp, vp]
    L.orbx_kfdb_detect_loop_frame.argtypes = [vp, vp, i, vp, i, f, vp, i, ip, vp, vp]
    L.orbx_kfdb_detect_relocalization_batch_device.argtypes = [vp, vp, i, vp, i, vp, vp]
    L.orbx_kfdb_reloc_scores.argtypes = [vp, vp, i]
    L.orbx_bow_frames_set_bow.argtypes = [vp, i, vp, vp, i, vp]
    L.orbx_undistort_keypoints.argtypes = [i, vp, i, f, f, f, f, vp, i, vp]
    L.orbx_rectifier_create.argtypes = [i, i, i, i, i, vp, vp, C.POINTER(vp)]
    L.orbx_rectifier_destroy.argtypes = [vp]; L.orbx_rectifier_destroy.restype = None
    L.orbx_rectifier_size.argtypes = [vp, ip, ip]
    L.orbx_remap_batch_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, i, vp, C.c_size_t, C.c_size_t, vp]
    L.orbx_extract_rectified.argtypes = [vp, vp, vp, i, i, C.c_size_t, vp, vp, i, ip, vp, C.c_size_t]
    RP = C.POINTER(RGBDParamsStruct)
    L.orbx_extract_rgbd.argtypes = [vp, vp, i, i, sz, i, i, vp, sz, RP, vp, vp, i, ip, vp, vp, vp]
    L.orbx_extract_rgbd_submit.argtypes = [vp, vp, i, i, sz, i, i, vp, sz, RP, ip]
    L.orbx_extract_rgbd_wait.argtypes = [vp, i, vp, vp, i, ip, vp, vp, vp]
    L.orbx_rgbd_depth_batch_device.argtypes = [i, vp, vp, i, i, vp, sz, sz, i, i, RP, vp, vp, vp, vp]
    L.orbx_search_for_initialization.argtypes = [i, C.POINTER(FrameFeats), C.POINTER(FrameFeats), vp, i, f, i, vp, ip]
    L.orbx_search_by_sim3.argtypes = [i, C.POINTER(FrameFeats), C.POINTER(FrameFeats), C.POINTER(ProjPoints), C.POINTER(ProjPoints),
                                      vp, vp, i, f, vp, ip]
    L.orbx_distinctive_descriptors.argtypes = [i, vp, vp, i, vp]
    L.orbx_profile_enable.argtypes = [vp, i]
    L.orbx_profile_stages.argtypes = [vp, C.c_uint]
    L.orbx_profile_read.argtypes = [vp, vp, vp, i]
    L.orbx_debug_candidates.argtypes = [vp, i, i, vp, vp, vp, i, ip]
    L.orbx_debug_level_counts.argtypes = [vp, i, vp]
    L.orbx_debug_fast_form.argtypes = [vp]
    L.orbx_debug_launch_forms.argtypes = [vp, vp, i]
    L.orbx_debug_fast_lane_table.argtypes = [i, i, i, vp, vp]
    L.orbx_debug_fast_cells.argtypes = [vp, vp, i]
    L.orbx_debug_bow_last_form.argtypes = [vp]
    L.orbx_debug_set_bow_form.argtypes = [i]
    L.orbx_debug_set_match_items.argtypes = [i]
    L.orbx_debug_match_timing.argtypes = [vp]
    L.orbx_thread_release.argtypes = []; L.orbx_thread_release.restype = None
    L.orbx_debug_thread_contexts.argtypes = []; L.orbx_debug_thread_contexts.restype = i
    _lib = L
    return L


def device_identity(device):
    """"<pci bus id> <uuid hex> <gcn arch>" of a visible device (orbx_device_identity)"""
    buf = C.create_string_buffer(160)
    _check(lib().orbx_device_identity(int(device), buf, len(buf)))
    return buf.value.decode(errors="replace")


def pipeline_depth():
    return lib().orbx_pipeline_depth()


class _Pinned:
    def __init__(self, nbytes):
        self.ptr = lib().orbx_pinned_alloc(nbytes)
        if not self.ptr:
            raise OrbxError(-5, lib().orbx_last_error().decode(errors="replace"))

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().orbx_pinned_free(self.ptr); self.ptr = None


def pinned_array(shape, dtype=np.uint8):
    """numpy array in page-locked host memory (orbx_pinned_alloc): uploads from it need no staging copy"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    owner = _Pinned(nbytes)
    buf = (C.c_uint8 * nbytes).from_address(owner.ptr)
    buf._orbx_owner = owner              # the ctypes buffer is the base object of every view: the pages are freed with the last of them
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


CV_TAPS_257, CV_TAPS_256 = 0, 1                 # named by what they are: the 7 taps sum to 257 (cvRound(k * 256)) or to 256 (error-diffused)
CV_PROFILE_3_2, CV_PROFILE_3_4_2 = 0, 1         # older names; which OpenCV release has which table is parity unpinned (include/orbx.h)


def gaussian_taps(profile):
    t = np.zeros(7, np.int32)
    _check(lib().orbx_gaussian_taps(profile, _p(t)))
    return t


def desc_rowpass_matrix(profile):
    """(B, acc0) of k_desc's matrix-core row pass: B[tile, lane, j] uint8 in the instruction's lane layout (orbx_desc_rowpass_matrix)"""
    b = np.zeros((3, 64, 16), np.uint8)
    acc0 = C.c_int(0)
    _check(lib().orbx_desc_rowpass_matrix(profile, _p(b), C.byref(acc0)))
    return b, acc0.value


def debug_fast_lane_table(tile_pitch, dw, dh):
    """k_fast's host-built lane table of one detect shape (orbx_debug_fast_lane_table): (entries uint32 [64, 4], rpi, half_mode); no device needed"""
    out = np.zeros((64, 4), np.uint32)
    uni = np.zeros(2, np.int32)
    _check(lib().orbx_debug_fast_lane_table(int(tile_pitch), int(dw), int(dh), _p(out), _p(uni)))
    return out, int(uni[0]), bool(uni[1])


def debug_set_bow_form(form):
    """test hook: "auto" / "wave" / "table" form of the SearchByBoW kernels (orbx_debug_set_bow_form)"""
    _check(lib().orbx_debug_set_bow_form({"auto": 0, "wave": 1, "table": 2}[form]))


def debug_bow_last_form():
    """form of the process's most recent SearchByBoW launch (orbx_debug_bow_last_form): dict with form ("wave" / "table" / None),
    xcd_grid and compact (bools)"""
    out = np.zeros(3, np.int32)
    _check(lib().orbx_debug_bow_last_form(_p(out)))
    return dict(form={0: None, 1: "wave", 2: "table"}[int(out[0])], xcd_grid=bool(out[1]), compact=bool(out[2]))


def thread_release():
    """give back, now, what the calling thread holds for the per-call searches on every device: streams, pinned and device staging
    (orbx_thread_release); a thread that ends does the same on its own"""
    lib().orbx_thread_release()


def debug_thread_contexts():
    """set-up per-thread search contexts of the whole process (orbx_debug_thread_contexts): one per (thread, family, device) in use"""
    return lib().orbx_debug_thread_contexts()


def debug_set_match_items(in_memory):
    """test hook: single-pair matcher calls read their work items from mapped host memory (True) or get them by value (False, default)"""
    _check(lib().orbx_debug_set_match_items(1 if in_memory else 0))


def _check(rc):
    if rc != 0:
        raise OrbxError(rc, lib().orbx_last_error().decode(errors="replace"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def make_featset(fs):
    """dict(desc[n,32]u8, node_id u32, node_off i32, feat u32, flag u8, angle f32[, x, y, octave, u_right])
    -> (FeatSet, keepalive dict)"""
    keep = {}

    def arr(k, dt):
        v = fs.get(k)
        if v is None:
            return None
        keep[k] = np.ascontiguousarray(v, dtype=dt)
        return keep[k].ctypes.data

    s = FeatSet()
    s.desc = arr("desc", np.uint8)
    s.n = len(keep["desc"])
    s.node_id = arr("node_id", np.uint32); s.node_off = arr("node_off", np.int32); s.feat = arr("feat", np.uint32)
    s.nnodes = len(keep["node_id"])
    s.flag = arr("flag", np.uint8); s.angle = arr("angle", np.float32)
    s.x = arr("x", np.float32); s.y = arr("y", np.float32)
    s.octave = arr("octave", np.int32); s.u_right = arr("u_right", np.float32)
    return s, keep


class ORBextractor:
    """Mirror of ORB_SLAM2::ORBextractor (reference include/ORBextractor.h:58-139).

    ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) as in src/Tracking.cc:124-130;
    `device`, `max_size`, `max_batch` size the HBM workspace.
    """

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device=0, max_size=(4096, 4096), max_batch=1):
        self._L = lib()
        self._h = C.c_void_p()
        self.nfeatures, self.nlevels, self.max_batch, self.device = nfeatures, nlevels, max_batch, device
        self._pipe_shapes, self._pipe_last = {}, (max_size[0], max_size[1])   # image sizes of the tickets in flight (pipelined forms)
        _check(self._L.orbx_extractor_create(C.byref(self._h), nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST,
                                             device, max_size[0], max_size[1], max_batch))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.orbx_extractor_destroy(h)
            self._h = None

    # -- getters (include/ORBextractor.h:78-98)
    def set_cv_profile(self, profile):
        """which OpenCV generation's GaussianBlur the descriptors are computed on: CV_PROFILE_3_2 (default) or CV_PROFILE_3_4_2"""
        _check(self._L.orbx_extractor_set_cv_profile(self._h, profile))

    def set_pyramid_group_limit(self, max_images):
        """tuning only (results do not change): launches of at most max_images images build several pyramid levels per launch; 0 = never"""
        _check(self._L.orbx_extractor_set_pyramid_group_limit(self._h, int(max_images)))

    def pipeline_warm(self, w, h):
        """make and touch every pipeline slot / kernel lane of the pipelined forms for w x h images now (orbx_pipeline_warm)"""
        _check(self._L.orbx_pipeline_warm(self._h, int(w), int(h)))

    def debug_fast_form(self):
        """1 = k_fast, 2 = k_fast2 (a pair of cells per wave) ran in the most recent extraction"""
        return self._L.orbx_debug_fast_form(self._h)

    FAST_CELL_FIELDS = ("level", "skip", "ini_x", "ini_y", "tw", "th", "pitch", "shape_class")

    def debug_fast_cells(self):
        """the FAST cell records of the current geometry (orbx_debug_fast_cells): int32 [cells, 8], columns FAST_CELL_FIELDS"""
        n = self._L.orbx_debug_fast_cells(self._h, None, 0)
        _check(min(n, 0))
        out = np.zeros((n, 8), np.int32)
        if n:
            _check(min(self._L.orbx_debug_fast_cells(self._h, _p(out), n), 0))
        return out

    LAUNCH_FORM_FIELDS = ("pyramid_regime", "fast_waves", "fast_image_major", "tree_threads", "tree_tab_lds", "tree_reg",
                          "desc_levels", "stereo_kpw", "stereo_xcd_grid", "desc_rowpass")

    def debug_launch_forms(self):
        """the form each size- and geometry-dependent launch took in the most recent extraction and in the most recent stereo
        launch with this handle as the left eye (orbx_debug_launch_forms), as a dict keyed by LAUNCH_FORM_FIELDS"""
        out = np.zeros(len(self.LAUNCH_FORM_FIELDS), np.int32)
        _check(min(self._L.orbx_debug_launch_forms(self._h, _p(out), len(out)), 0))
        return dict(zip(self.LAUNCH_FORM_FIELDS, (int(v) for v in out)))

    def GetLevels(self): return self._L.orbx_get_levels(self._h)
    def GetScaleFactor(self): return self._L.orbx_get_scale_factor(self._h)

    def _tables(self):
        t = [np.zeros(self.nlevels, np.float32) for _ in range(4)]
        _check(self._L.orbx_get_scale_tables(self._h, *[_p(a) for a in t]))
        return t

    def GetScaleFactors(self): return self._tables()[0]
    def GetInverseScaleFactors(self): return self._tables()[1]
    def GetScaleSigmaSquares(self): return self._tables()[2]
    def GetInverseScaleSigmaSquares(self): return self._tables()[3]

    def GetFeaturesPerLevel(self):
        q = np.zeros(self.nlevels, np.int32)
        _check(self._L.orbx_get_features_per_level(self._h, _p(q)))
        return q

    def max_keypoints(self, w, h):
        n = self._L.orbx_max_keypoints(self._h, w, h)
        if n < 0:
            _check(n)
        return n

    # -- operator() (include/ORBextractor.h:74-76): image -> (keypoints, descriptors)
    def __call__(self, image, mask=None):
        image = np.asarray(image)
        if image.size == 0:
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        if image.dtype != np.uint8 or image.ndim != 2:
            raise OrbxError(-1, "image must be 2-D uint8 (CV_8UC1, reference src/ORBextractor.cc:1269)")
        if image.strides[1] != 1:
            image = np.ascontiguousarray(image)
        h, w = image.shape
        cap = self.max_keypoints(w, h)
        kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); n = C.c_int()
        _check(self._L.orbx_extract(self._h, _p(image), w, h, image.strides[0], _p(kps), _p(desc), cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_stereo(self, imLeft, imRight, bf, min_z):
        """one stereo frame in one call: both eyes' operator() + Frame::ComputeStereoMatches (reference src/Frame.cc:82-97)
        -> (kpsL, descL, kpsR, descR, uRight, depth); the extractor needs max_batch >= 2"""
        L_ = np.ascontiguousarray(imLeft, np.uint8); R_ = np.ascontiguousarray(imRight, np.uint8)
        if L_.shape != R_.shape or L_.ndim != 2:
            raise OrbxError(-1, "left and right image must be equal 2-D uint8 arrays")
        h, w = L_.shape
        cap = self.max_keypoints(w, h)
        kps = np.zeros((2, cap), KP_DTYPE); desc = np.zeros((2, cap, 32), np.uint8); n = np.zeros(2, np.int32)
        ur = np.zeros(cap, np.float32); z = np.zeros(cap, np.float32)
        _check(self._L.orbx_extract_stereo(self._h, _p(L_), _p(R_), w, h, L_.strides[0], bf, min_z, _p(kps), _p(desc), cap, _p(n), _p(ur), _p(z)))
        return (kps[0, :n[0]].copy(), desc[0, :n[0]].copy(), kps[1, :n[1]].copy(), desc[1, :n[1]].copy(), ur[:n[0]].copy(), z[:n[0]].copy())

    def extract_submit(self, image):
        """pipelined monocular form of __call__ -> ticket"""
        if image.ndim != 2 or image.dtype != np.uint8 or image.strides[1] != 1:
            raise OrbxError(-1, "image must be a 2-D uint8 array with unit column stride")
        h, w = image.shape
        t = C.c_int()
        _check(self._L.orbx_extract_submit(self._h, image.ctypes.data, w, h, image.strides[0], C.byref(t)))
        self._pipe_shapes[t.value] = (w, h); self._pipe_last = (w, h)
        return t.value

    def extract_wait(self, ticket):
        w, h = self._pipe_shapes.pop(ticket, self._pipe_last)       # an unknown ticket is the library's error to report
        cap = self.max_keypoints(w, h)
        kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); n = C.c_int()
        _check(self._L.orbx_extract_wait(self._h, ticket, _p(kps), _p(desc), cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    # -- pipelined form: up to pipeline_depth() frames in flight, uploads / downloads overlap the kernels of the neighbouring frames
    def extract_stereo_submit(self, imLeft, imRight, bf, min_z):
        """-> ticket; the images are copied (or, if they live in pinned_array() memory, must stay untouched until the wait)"""
        if imLeft.shape != imRight.shape or imLeft.ndim != 2 or imLeft.dtype != np.uint8 or imLeft.strides != imRight.strides or imLeft.strides[1] != 1:
            raise OrbxError(-1, "left and right image must be equal 2-D uint8 arrays with unit column stride")
        h, w = imLeft.shape
        t = C.c_int()
        _check(self._L.orbx_extract_stereo_submit(self._h, imLeft.ctypes.data, imRight.ctypes.data, w, h, imLeft.strides[0], bf, min_z, C.byref(t)))
        self._pipe_shapes[t.value] = (w, h); self._pipe_last = (w, h)
        return t.value

    def extract_stereo_wait(self, ticket, copy=True):
        w, h = self._pipe_shapes.pop(ticket, self._pipe_last)       # an unknown ticket is the library's error to report
        cap = self.max_keypoints(w, h)
        b = getattr(self, "_pipe_out", None)
        if b is None or b[0].shape[1] != cap:
            b = self._pipe_out = (np.zeros((2, cap), KP_DTYPE), np.zeros((2, cap, 32), np.uint8), np.zeros(2, np.int32),
                                  np.zeros(cap, np.float32), np.zeros(cap, np.float32))
        kps, desc, n, ur, z = b
        _check(self._L.orbx_extract_stereo_wait(self._h, ticket, _p(kps), _p(desc), cap, _p(n), _p(ur), _p(z)))
        if not copy:      # views into buffers that the next wait overwrites (measurement loops)
            return kps[0, :n[0]], desc[0, :n[0]], kps[1, :n[1]], desc[1, :n[1]], ur[:n[0]], z[:n[0]]
        return (kps[0, :n[0]].copy(), desc[0, :n[0]].copy(), kps[1, :n[1]].copy(), desc[1, :n[1]].copy(), ur[:n[0]].copy(), z[:n[0]].copy())

    # -- RGB-D: Tracking::GrabImageRGBD's image preparation + Frame::Frame(imGray, imDepth, ...) up to ComputeStereoFromRGBD
    #    (reference src/Tracking.cc:217-233, src/Frame.cc:145-154)
    def extract_rgbd(self, image, depth, params, rgb=True):
        """grey (H x W) or colour (H x W x 3|4, rgb = Camera.RGB) uint8 image + uint16 / float32 depth map, RGBDParams
        -> (keypoints, descriptors, xy_un [n, 2], uRight, depth)"""
        image, ch = _rgbd_image(image)
        depth = _rgbd_depth(depth)
        h, w = image.shape[:2]
        if depth.shape != (h, w):
            raise OrbxError(-1, "depth map and image differ in size")
        p = params.struct(_depth_type(depth))
        cap = self.max_keypoints(w, h)
        kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); n = C.c_int()
        xy = np.zeros((cap, 2), np.float32); ur = np.zeros(cap, np.float32); z = np.zeros(cap, np.float32)
        _check(self._L.orbx_extract_rgbd(self._h, _p(image), w, h, image.strides[0], ch, int(rgb), _p(depth), depth.strides[0], C.byref(p),
                                         _p(kps), _p(desc), cap, C.byref(n), _p(xy), _p(ur), _p(z)))
        k = n.value
        return kps[:k].copy(), desc[:k].copy(), xy[:k].copy(), ur[:k].copy(), z[:k].copy()

    def extract_rgbd_submit(self, image, depth, params, rgb=True):
        """pipelined form of extract_rgbd -> ticket; image / depth are copied (or, if they live in pinned_array() memory with dense rows,
        read in place and must stay untouched until the wait)"""
        image, ch = _rgbd_image(image)
        depth = _rgbd_depth(depth)
        h, w = image.shape[:2]
        if depth.shape != (h, w):
            raise OrbxError(-1, "depth map and image differ in size")
        p = params.struct(_depth_type(depth))
        t = C.c_int()
        _check(self._L.orbx_extract_rgbd_submit(self._h, image.ctypes.data, w, h, image.strides[0], ch, int(rgb), depth.ctypes.data,
                                                depth.strides[0], C.byref(p), C.byref(t)))
        self._pipe_shapes[t.value] = (w, h); self._pipe_last = (w, h)
        return t.value

    def extract_rgbd_wait(self, ticket):
        """-> (keypoints, descriptors, xy_un, uRight, depth) of an extract_rgbd_submit ticket"""
        w, h = self._pipe_shapes.pop(ticket, self._pipe_last)       # an unknown ticket is the library's error to report
        cap = self.max_keypoints(w, h)
        kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); n = C.c_int()
        xy = np.zeros((cap, 2), np.float32); ur = np.zeros(cap, np.float32); z = np.zeros(cap, np.float32)
        _check(self._L.orbx_extract_rgbd_wait(self._h, ticket, _p(kps), _p(desc), cap, C.byref(n), _p(xy), _p(ur), _p(z)))
        k = n.value
        return kps[:k].copy(), desc[:k].copy(), xy[:k].copy(), ur[:k].copy(), z[:k].copy()

    def extract_color(self, image, rgb=True, want_gray=False):
        """colour frame (H x W x 3|4 uint8): cvtColor to grey on device (Tracking::GrabImage*, src/Tracking.cc:177-202), then operator()"""
        image = np.ascontiguousarray(image, np.uint8)
        h, w, ch = image.shape
        cap = self.max_keypoints(w, h)
        kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); n = C.c_int()
        gray = np.zeros((h, w), np.uint8) if want_gray else None
        _check(self._L.orbx_extract_color(self._h, _p(image), w, h, image.strides[0], ch, int(rgb), _p(kps), _p(desc), cap, C.byref(n),
                                          _p(gray), gray.strides[0] if want_gray else 0))
        out = (kps[:n.value].copy(), desc[:n.value].copy())
        return out + (gray,) if want_gray else out

    def extract_rectified(self, rectifier, image, want_rect=False):
        """raw grey frame -> cv::remap on device (Examples/Stereo/stereo_euroc.cc:136-137) -> operator()"""
        image = np.ascontiguousarray(image, np.uint8)
        h, w = image.shape
        rw, rh = rectifier.size
        cap = self.max_keypoints(rw, rh)
        kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); n = C.c_int()
        rect = np.zeros((rh, rw), np.uint8) if want_rect else None
        _check(self._L.orbx_extract_rectified(self._h, rectifier._h, _p(image), w, h, image.strides[0], _p(kps), _p(desc), cap, C.byref(n),
                                              _p(rect), rect.strides[0] if want_rect else 0))
        out = (kps[:n.value].copy(), desc[:n.value].copy())
        return out + (rect,) if want_rect else out

    def extract_batch(self, images):
        """list/array of equally sized uint8 images -> list of (keypoints, descriptors)"""
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        h, w = imgs[0].shape
        B = len(imgs)
        cap = self.max_keypoints(w, h)
        ptrs = (C.c_void_p * B)(*[im.ctypes.data for im in imgs])
        kps = np.zeros((B, cap), KP_DTYPE); desc = np.zeros((B, cap, 32), np.uint8); n = np.zeros(B, np.int32)
        _check(self._L.orbx_extract_batch(self._h, ptrs, B, w, h, imgs[0].strides[0], _p(kps), _p(desc), cap, _p(n)))
        return [(kps[i, :n[i]].copy(), desc[i, :n[i]].copy()) for i in range(B)]

    def extract_batch_device(self, d_imgs, img_stride, pitch, batch, w, h, d_kps, d_desc, cap, d_n, stream=None):
        """device pointers (ints); asynchronous on `stream` (None = the handle's own)"""
        _check(self._L.orbx_extract_batch_device(self._h, d_imgs, img_stride, pitch, batch, w, h, d_kps, d_desc, cap, d_n, stream))

    def sync(self, stream=None):
        _check(self._L.orbx_sync(self._h, stream))

    # -- mvImagePyramid (include/ORBextractor.h:100)
    def pyramid_level(self, level, image_index=0):
        w, h = C.c_int(), C.c_int()
        _check(self._L.orbx_pyramid_level(self._h, image_index, level, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _check(self._L.orbx_pyramid_level(self._h, image_index, level, _p(out), out.strides[0], C.byref(w), C.byref(h)))
        return out

    @property
    def mvImagePyramid(self):
        return [self.pyramid_level(l) for l in range(self.nlevels)]

    # -- inspection / measurement
    def debug_candidates(self, level, image_index=0):
        n = C.c_int()
        _check(self._L.orbx_debug_candidates(self._h, image_index, level, None, None, None, 0, C.byref(n)))
        x = np.zeros(n.value, np.int32); y = np.zeros(n.value, np.int32); r = np.zeros(n.value, np.int32)
        _check(self._L.orbx_debug_candidates(self._h, image_index, level, _p(x), _p(y), _p(r), n.value, C.byref(n)))
        return x, y, r

    def debug_level_counts(self, image_index=0):
        c = np.zeros(self.nlevels, np.int32)
        _check(self._L.orbx_debug_level_counts(self._h, image_index, _p(c)))
        return c

    def profile_enable(self, on=True):
        _check(self._L.orbx_profile_enable(self._h, int(on)))

    def profile_stages(self, mask=0xFFFFFFFF):
        """which stages record events while profiling is on (bit = ORBX_STAGE_*; default all)"""
        _check(self._L.orbx_profile_stages(self._h, int(mask) & 0xFFFFFFFF))

    def profile_read(self, reset=True):
        ms = np.zeros(len(STAGES), np.float32); n = np.zeros(len(STAGES), np.int32)
        _check(self._L.orbx_profile_read(self._h, _p(ms), _p(n), int(reset)))
        return {s: (float(ms[i]), int(n[i])) for i, s in enumerate(STAGES)}


def ComputeStereoMatches(extractorLeft, extractorRight, mvKeys, mDescriptors, mvKeysRight, mDescriptorsRight, mbf, mb):
    """Mirror of Frame::ComputeStereoMatches (reference src/Frame.cc:577-751) -> (mvuRight, mvDepth).
    `mb` is the stereo baseline in metres (minZ); the reference reads it uninitialised."""
    kL = np.ascontiguousarray(mvKeys, dtype=KP_DTYPE); kR = np.ascontiguousarray(mvKeysRight, dtype=KP_DTYPE)
    dL = np.ascontiguousarray(mDescriptors, dtype=np.uint8); dR = np.ascontiguousarray(mDescriptorsRight, dtype=np.uint8)
    ur = np.full(len(kL), -1, np.float32); dp = np.full(len(kL), -1, np.float32)
    _check(lib().orbx_stereo_match(extractorLeft._h, extractorRight._h, _p(kL), _p(dL), len(kL), _p(kR), _p(dR), len(kR),
                                   mbf, mb, _p(ur), _p(dp)))
    return ur, dp


ROWTAB_FROM_KEYPOINTS, ROWTAB_OF_EXTRACTION = 0, 1


def stereo_match_batch_device(L, imgL0, R, imgR0, batch, d_kL, d_dL, d_nL, d_kR, d_dR, d_nR, cap, bf, min_z, d_ur, d_depth, stream=None,
                              row_table=ROWTAB_FROM_KEYPOINTS):
    """row_table: ROWTAB_FROM_KEYPOINTS (always correct: the table is built from d_kR) or ROWTAB_OF_EXTRACTION (the caller asserts that
    d_kR still holds what R's last extract_batch_device wrote: that launch's by-product table is used; refused if it cannot be)"""
    _check(lib().orbx_stereo_match_batch_device(L._h, imgL0, R._h, imgR0, batch, d_kL, d_dL, d_nL, d_kR, d_dR, d_nR, cap,
                                                bf, min_z, d_ur, d_depth, row_table, stream))


def rgbd_depth_batch_device(device, d_kps, d_n, cap, batch, d_depth, depth_img_stride, depth_pitch, w, h, params, depth_type,
                            d_u_right, d_depth_out, d_xy_un=None, stream=None):
    """orbx_rgbd_depth_batch_device: UndistortKeyPoints + ComputeStereoFromRGBD (reference src/Frame.cc:152-154) for `batch` images of
    orbx_extract_batch_device's outputs; device pointers (ints), outputs [batch*cap]; entries at or beyond a count stay untouched.
    Asynchronous on `stream`."""
    p = params.struct(depth_type)
    _check(lib().orbx_rgbd_depth_batch_device(int(device), d_kps, d_n, int(cap), int(batch), d_depth, int(depth_img_stride), int(depth_pitch),
                                              int(w), int(h), C.byref(p), d_xy_un, d_u_right, d_depth_out, stream))


def stereo_row_table_available(R, d_kR, imgR0, batch, cap):
    return bool(lib().orbx_stereo_row_table_available(R._h, d_kR, imgR0, batch, cap))


class ORBVocabulary:
    """Mirror of ORB_SLAM2::ORBVocabulary (= DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>, reference
    include/ORBVocabulary.h) for the part on the hot path: loadFromTextFile and transform()."""

    def __init__(self, k=None, L=None, parent=None, is_leaf=None, desc=None, weight=None, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        if k is not None:
            parent = np.ascontiguousarray(parent, np.int32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
            desc = np.ascontiguousarray(desc, np.uint8); weight = np.ascontiguousarray(weight, np.float64)
            _check(self._L.orbx_vocab_create(device, k, L, len(parent), _p(parent), _p(is_leaf), _p(desc), _p(weight), C.byref(self._h)))

    @classmethod
    def loadFromTextFile(cls, filename, device=0):
        v = cls(device=device)
        _check(v._L.orbx_vocab_load_text(device, str(filename).encode(), C.byref(v._h)))
        return v

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.orbx_vocab_destroy(h)
            self._h = None

    def info(self):
        k, L_, n, w = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _check(self._L.orbx_vocab_info(self._h, C.byref(k), C.byref(L_), C.byref(n), C.byref(w)))
        return dict(k=k.value, L=L_.value, nodes=n.value, words=w.value)

    def transform(self, features, levelsup=4):
        """-> dict(word_id, word_weight, node_id, bow_id, bow_val, fv_node_id, fv_node_off, fv_feat)"""
        desc = np.ascontiguousarray(features, np.uint8).reshape(-1, 32); n = len(desc)
        wid = np.zeros(n, np.uint32); ww = np.zeros(n, np.float64); nid = np.zeros(n, np.uint32)
        bid = np.zeros(n, np.uint32); bval = np.zeros(n, np.float64); nb = C.c_int()
        fid = np.zeros(n, np.uint32); foff = np.zeros(n + 1, np.int32); ffeat = np.zeros(n, np.uint32); fn = C.c_int()
        _check(self._L.orbx_bow_transform(self._h, _p(desc), n, levelsup, _p(wid), _p(ww), _p(nid), _p(bid), _p(bval), C.byref(nb),
                                          _p(fid), _p(foff), _p(ffeat), C.byref(fn)))
        return dict(word_id=wid, word_weight=ww, node_id=nid, bow_id=bid[:nb.value].copy(), bow_val=bval[:nb.value].copy(),
                    fv_node_id=fid[:fn.value].copy(), fv_node_off=foff[:fn.value + 1].copy(), fv_feat=ffeat[:foff[fn.value]].copy())


class DeviceKeyFrame:
    """orbx_kf: a keyframe's (or frame's) immutable matching data resident in HBM in FeatureVector order: descriptors,
    FeatureVector, angles and, when given, positions / octaves / u_right.  Map-point flags are passed per search."""

    def __init__(self, fs, device=0):
        s, keep = make_featset(fs)
        h = C.c_void_p()
        _check(lib().orbx_kf_create(device, C.byref(s), C.byref(h)))
        self._h, self.n, self.device = h, s.n, device

    def __del__(self):
        # at interpreter shutdown the module globals (and ctypes itself) may already be torn down: never raise from a finaliser
        try:
            h, L = getattr(self, "_h", None), _lib
            if h and L is not None:
                L.orbx_kf_destroy(h)
            self._h = None
        except Exception:
            pass


def _flags_for(flag, kf, who):
    """per-feature flag array of a resident keyframe: one byte per feature of THAT keyframe (the library reads kf.n bytes)"""
    fl = np.ascontiguousarray(flag, np.uint8)
    if fl.ndim != 1 or len(fl) != kf.n:
        raise OrbxError(-1, f"{who}: flag array has {fl.size} entries, the keyframe has {kf.n} features")
    return fl


class DeviceFrame:
    """orbx_frame: the current frame's immutable part resident in HBM -- undistorted x / y, octave, angle, u_right, descriptors, bounds and
    the 64x48 grid, built once -- for the two to four projection searches Tracking runs on it.  `occupied` is passed per search."""

    def __init__(self, frame, device=0):
        s_, keep = ORBmatcher._frame(dict(frame, occupied=None))
        h = C.c_void_p()
        _check(lib().orbx_frame_create(device, C.byref(s_), C.byref(h)))
        self._h, self.n, self.device = h, s_.n, device

    @classmethod
    def from_extraction(cls, device, d_kps, d_desc, d_n, cap, index, d_u_right=None, K=None, dist_coef=None, bounds=(0.0, 0.0, 0.0, 0.0),
                        stream=None):
        """from orbx_extract_batch_device's device outputs (image `index`, capacity `cap`) and optionally the [cap] u_right row of
        orbx_stereo_match_batch_device; K = (fx, fy, cx, cy) with dist_coef undistorts on the device.  Synchronises `stream` once (the count)."""
        kk = None if K is None else np.ascontiguousarray(K, np.float32).reshape(4)
        dc = None if dist_coef is None else np.ascontiguousarray(dist_coef, np.float32).reshape(-1)
        h = C.c_void_p()
        _check(lib().orbx_frame_create_from_extraction(device, d_kps, d_desc, d_n, int(cap), int(index), d_u_right,
                                                       None if kk is None else _p(kk), None if dc is None else _p(dc), 0 if dc is None else len(dc),
                                                       *[float(v) for v in bounds], stream, C.byref(h)))
        self = cls.__new__(cls)
        self._h, self.device = h, device
        self.n = lib().orbx_frame_size(h)
        self.bounds = tuple(float(v) for v in bounds)
        return self

    def read(self):
        """-> dict(x, y, octave, angle, u_right, desc) as tests/test_projection.py builds a frame (no occupied, no bounds)"""
        n = self.n
        x = np.zeros(n, np.float32); y = np.zeros(n, np.float32); o = np.zeros(n, np.int32); a = np.zeros(n, np.float32)
        u = np.zeros(n, np.float32); d = np.zeros((n, 32), np.uint8)
        _check(lib().orbx_frame_read(self._h, _p(x), _p(y), _p(o), _p(a), _p(u), _p(d)))
        return dict(x=x, y=y, octave=o, angle=a, u_right=u, desc=d)

    def search_local_points(self, occupied, points, slots, flags, pose, cam, view_cos_limit, log_scale_factor, scaleFactors, th=1.0,
                            nnratio=0.8):
        """Tracking::SearchLocalPoints' second loop and matcher call on slots of a MapPoints table: flags bit 0 = eligible, bit 1 =
        Observations() > 0 -> (match_cur, nmatches, in_view)"""
        oc = _occupied_for(occupied, self, "DeviceFrame.search_local_points")
        sl = MapPoints._slots(slots)
        fl = np.ascontiguousarray(flags, np.uint8)
        if fl.shape != sl.shape:
            raise OrbxError(-1, f"DeviceFrame.search_local_points: {len(sl)} slots, {fl.size} flag bytes")
        po, ca = _pose_cam(pose, cam, "DeviceFrame.search_local_points")
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        out = np.full(self.n, -1, np.int32); n = C.c_int(); iv = np.zeros(len(sl), np.uint8)
        _check(lib().orbx_frame_search_local_points(self._h, None if oc is None else _p(oc), points._h, _p(sl), _p(fl), len(sl), _p(po), _p(ca),
                                                    float(view_cos_limit), float(log_scale_factor), _p(sf), len(sf), float(th), float(nnratio),
                                                    _p(out), C.byref(n), _p(iv)))
        return out, n.value, iv

    def pose_optimize(self, points, slot_of_feature, invLevelSigma2, cam, Tcw):
        """Optimizer::PoseOptimization on this frame and a MapPoints table: slot_of_feature[n] names each feature's point (-1: none)
        -> dict as pose_optimize (outlier is 0 where a feature has no point)"""
        sl = MapPoints._slots(slot_of_feature)
        if len(sl) != self.n:
            raise OrbxError(-1, f"DeviceFrame.pose_optimize: {len(sl)} slots, the frame has {self.n} features")
        isig = np.ascontiguousarray(invLevelSigma2, np.float32).reshape(-1)
        ca, tc = _pose_inputs(cam, Tcw, "DeviceFrame.pose_optimize")
        out = np.zeros(16, np.float32); fl = np.zeros(self.n, np.uint8); ni = C.c_int(); rep = PoseReport()
        _check(lib().orbx_frame_pose_optimize(self._h, points._h, _p(sl), _p(isig), len(isig), _p(ca), _p(tc), _p(out), _p(fl), C.byref(ni),
                                              C.byref(rep)))
        return _pose_result(out, fl, ni.value, rep)

    def __del__(self):
        try:
            h, L = getattr(self, "_h", None), _lib
            if h and L is not None:
                L.orbx_frame_destroy(h)
            self._h = None
        except Exception:
            pass


class MapPoints:
    """orbx_mappoints: the map points' position, normal, distance range and descriptor resident in HBM, a slot per point, in a table of
    fixed capacity.  frustum() is Frame::isInFrustum from a pose; DeviceFrame.search_local_points fuses it with the map-point search."""

    def __init__(self, capacity, device=0):
        h = C.c_void_p()
        _check(lib().orbx_mappoints_create(device, int(capacity), C.byref(h)))
        self._h, self.device = h, device
        self.capacity = lib().orbx_mappoints_capacity(h)

    def __del__(self):
        try:
            h, L = getattr(self, "_h", None), _lib
            if h and L is not None:
                L.orbx_mappoints_destroy(h)
            self._h = None
        except Exception:
            pass

    @staticmethod
    def _slots(slots):
        sl = np.ascontiguousarray(slots, np.int32)
        if sl.ndim != 1:
            raise OrbxError(-1, "MapPoints: slots must be one-dimensional")
        return sl

    def set(self, slots, geom=None, desc=None, stream=None):
        """geom[n][8] = X Y Z mfMinDistance nx ny nz mfMaxDistance, desc[n][32]; either may be None to leave that half as it is"""
        sl = self._slots(slots)
        g = None if geom is None else np.ascontiguousarray(geom, np.float32)
        d = None if desc is None else np.ascontiguousarray(desc, np.uint8)
        if (g is not None and g.shape != (len(sl), 8)) or (d is not None and d.shape != (len(sl), 32)):
            raise OrbxError(-1, f"MapPoints.set: {len(sl)} slots need geom [{len(sl)}][8] and desc [{len(sl)}][32]")
        _check(lib().orbx_mappoints_set(self._h, _p(sl), len(sl), None if g is None else _p(g), None if d is None else _p(d), stream))

    def read(self, slots):
        """-> (geom[n][8], desc[n][32]) of the named slots"""
        sl = self._slots(slots)
        g = np.zeros((len(sl), 8), np.float32); d = np.zeros((len(sl), 32), np.uint8)
        _check(lib().orbx_mappoints_read(self._h, _p(sl), len(sl), _p(g), _p(d)))
        return g, d

    def frustum(self, slots, eligible, pose, cam, view_cos_limit, log_scale_factor, nlevels):
        """Frame::isInFrustum of the named slots; pose = Rcw[9] tcw[3] Ow[3], cam = fx fy cx cy mbf mnMinX mnMinY mnMaxX mnMaxY
        -> dict(in_view, u, v, xr, level, view_cos)"""
        sl = self._slots(slots)
        el = np.ascontiguousarray(eligible, np.uint8)
        if el.shape != sl.shape:
            raise OrbxError(-1, f"MapPoints.frustum: {len(sl)} slots, {el.size} eligible bytes")
        po, ca = _pose_cam(pose, cam, "MapPoints.frustum")
        n = len(sl)
        o = dict(in_view=np.zeros(n, np.uint8), u=np.zeros(n, np.float32), v=np.zeros(n, np.float32), xr=np.zeros(n, np.float32),
                 level=np.zeros(n, np.int32), view_cos=np.zeros(n, np.float32))
        _check(lib().orbx_mappoints_frustum(self._h, _p(sl), _p(el), n, _p(po), _p(ca), float(view_cos_limit), float(log_scale_factor),
                                            int(nlevels), _p(o["in_view"]), _p(o["u"]), _p(o["v"]), _p(o["xr"]), _p(o["level"]),
                                            _p(o["view_cos"])))
        return o


class MapGraph:
    """orbx_mapgraph: who observes what, resident in HBM in both views of the reference -- per keyframe slot and feature the point slot,
    octave, stereo bit and close bit (KeyFrame::mvpMapPoints), per point slot the (keyframe, feature) entries, nObs and a bad bit
    (MapPoint::mObservations).  Edited in small batches, one mutator of the reference each; vote() is keyframeCounter of
    Tracking::UpdateLocalKeyFrames, covisibility() KFcounter of KeyFrame::UpdateConnections, cull_keyframes() the loop of
    LocalMapping::KeyFrameCulling with its effects on the map applied between iterations."""

    def __init__(self, max_keyframes, max_features, max_points, max_obs=256, device=0):
        h = C.c_void_p()
        _check(lib().orbx_mapgraph_create(device, int(max_keyframes), int(max_features), int(max_points), int(max_obs), C.byref(h)))
        self._h, self.device = h, device
        self.max_keyframes, self.max_features, self.max_points, self.max_obs = int(max_keyframes), int(max_features), int(max_points), int(max_obs)

    def __del__(self):
        try:
            h, L = getattr(self, "_h", None), _lib
            if h and L is not None:
                L.orbx_mapgraph_destroy(h)
            self._h = None
        except Exception:
            pass

    @staticmethod
    def _cols(who, *cols):
        a = [np.ascontiguousarray(c, np.int32) for c in cols]
        if any(c.ndim != 1 or len(c) != len(a[0]) for c in a):
            raise OrbxError(-1, f"MapGraph.{who}: the lists must be one-dimensional and of one length")
        return a

    def clear(self):
        _check(lib().orbx_mapgraph_clear(self._h))

    def set_keyframe(self, kf, octave, stereo, close):
        """a new keyframe in the free slot kf: per feature its octave, whether mvuRight >= 0, whether 0 <= mvDepth <= mThDepth"""
        o, s, c = (np.ascontiguousarray(x, np.uint8) for x in (octave, stereo, close))
        if o.ndim != 1 or s.shape != o.shape or c.shape != o.shape:
            raise OrbxError(-1, "MapGraph.set_keyframe: octave, stereo and close must be one-dimensional and of one length")
        _check(lib().orbx_mapgraph_set_keyframe(self._h, int(kf), len(o), _p(o), _p(s), _p(c)))

    def set_matches(self, kf, idx, point):
        i, p = self._cols("set_matches", idx, point)
        _check(lib().orbx_mapgraph_set_matches(self._h, int(kf), _p(i), _p(p), len(i)))

    def add_observations(self, point, kf, idx):
        p, k, i = self._cols("add_observations", point, kf, idx)
        _check(lib().orbx_mapgraph_add_observations(self._h, _p(p), _p(k), _p(i), len(p)))

    def erase_observations(self, point, kf):
        p, k = self._cols("erase_observations", point, kf)
        _check(lib().orbx_mapgraph_erase_observations(self._h, _p(p), _p(k), len(p)))

    def erase_points(self, point):
        p, = self._cols("erase_points", point)
        _check(lib().orbx_mapgraph_erase_points(self._h, _p(p), len(p)))

    def erase_keyframe(self, kf):
        _check(lib().orbx_mapgraph_erase_keyframe(self._h, int(kf)))

    def keyframe_observations(self, kf):
        """the row entries that name keyframe slot kf, in use or free"""
        n = lib().orbx_mapgraph_keyframe_observations(self._h, int(kf))
        if n < 0:
            _check(n)
        return n

    def read_keyframe(self, kf):
        """-> None for a free slot, else dict(point, octave, stereo, close), from the device's copy"""
        n = C.c_int()
        p = np.zeros(self.max_features, np.int32)
        o, s, c = (np.zeros(self.max_features, np.uint8) for _ in range(3))
        _check(lib().orbx_mapgraph_read_keyframe(self._h, int(kf), C.byref(n), _p(p), _p(o), _p(s), _p(c)))
        if n.value < 0:
            return None
        return dict(point=p[:n.value], octave=o[:n.value], stereo=s[:n.value], close=c[:n.value])

    def read_points(self, first=0, n=None):
        """-> {slot: dict(n_obs, bad, obs = the row as a sorted list of (keyframe slot, feature index))} of the live slots among
        first .. first + n - 1, from the device's copy"""
        n = self.max_points - first if n is None else int(n)
        nobs, ne = np.zeros(n, np.int32), np.zeros(n, np.int32)
        fl = np.zeros(n, np.uint8)
        k, i = np.zeros((n, self.max_obs), np.int32), np.zeros((n, self.max_obs), np.int32)
        _check(lib().orbx_mapgraph_read_points(self._h, int(first), n, _p(nobs), _p(fl), _p(ne), _p(k), _p(i)))
        return {first + p: dict(n_obs=int(nobs[p]), bad=bool(fl[p] & 2), obs=sorted(zip(k[p, :ne[p]].tolist(), i[p, :ne[p]].tolist())))
                for p in np.flatnonzero(fl & 1).tolist()}

    def read_point(self, point):
        """-> dict(n_obs, bad, obs), or None for a slot that is not live"""
        return self.read_points(point, 1).get(int(point))

    def _counts(self):
        return np.zeros(self.max_keyframes, np.int32), np.zeros(self.max_keyframes, np.int32), C.c_int()

    def vote(self, points):
        """-> (counts[max_keyframes] by keyframe slot, the slots with a non-zero count)"""
        p, = self._cols("vote", points)
        cnt, nz, n = self._counts()
        _check(lib().orbx_mapgraph_vote(self._h, _p(p), len(p), _p(cnt), _p(nz), C.byref(n)))
        return cnt, nz[:n.value].copy()

    def covisibility(self, kf):
        """-> (counts[max_keyframes] over kf's own matches with kf left out, the slots with a non-zero count)"""
        cnt, nz, n = self._counts()
        _check(lib().orbx_mapgraph_covisibility(self._h, int(kf), _p(cnt), _p(nz), C.byref(n)))
        return cnt, nz[:n.value].copy()

    def cull_keyframes(self, local, not_erase, monocular, cap=None):
        """-> dict(culled[n] 0 / 1 culled / 2 mbToBeErased, n_mps[n], n_redundant[n], bad_points ascending)"""
        lo, = self._cols("cull_keyframes", local)
        ne = np.ascontiguousarray(not_erase, np.uint8)
        if ne.shape != lo.shape:
            raise OrbxError(-1, f"MapGraph.cull_keyframes: {len(lo)} keyframes, {ne.size} not_erase bytes")
        n = len(lo)
        cap = self.max_points if cap is None else int(cap)
        cu = np.zeros(n, np.uint8); mps = np.zeros(n, np.int32); red = np.zeros(n, np.int32)
        bad = np.zeros(max(cap, 1), np.int32); nb = C.c_int()
        rc = lib().orbx_mapgraph_cull_keyframes(self._h, _p(lo), _p(ne), n, 1 if monocular else 0, _p(cu), _p(mps), _p(red), _p(bad), cap, C.byref(nb))
        self.last_n_bad = nb.value
        _check(rc)
        return dict(culled=cu, n_mps=mps, n_redundant=red, bad_points=bad[:nb.value].copy())

    def refresh_points(self, points, *, table=None, table_slots=None, pos=None, ref_kf=None, keyframes=None, scale_factors=None,
                       what=REFRESH_GEOM | REFRESH_DESC, out=None, stream=None):
        """MapPoint::UpdateNormalAndDepth (what & 1) and ComputeDistinctiveDescriptors (what & 2) of the listed point slots, written into
        `table` (a MapPoints, slots table_slots or the point slots themselves) when there is one.  keyframes = dict(slot[nk], centre[nk][3],
        bad[nk], frame = nk DeviceFrames or None): every keyframe a row may name, and every ref_kf.  pos[n][3] = mWorldPos (None: as the table
        holds it).  out: a RefreshResult to write into (rows that are not updated stay as they are) -> RefreshResult"""
        who = "MapGraph.refresh_points"
        pt, = self._cols("refresh_points", points)
        n = len(pt)
        kf = keyframes or dict(slot=[], centre=np.zeros((0, 3)), bad=[], frame=[])
        ks = np.ascontiguousarray(kf["slot"], np.int32).reshape(-1)
        nk = len(ks)
        kc = np.ascontiguousarray(kf["centre"], np.float32).reshape(-1, 3)
        kb = np.ascontiguousarray(kf["bad"], np.uint8).reshape(-1)
        frames = list(kf.get("frame") or [None] * nk)
        if len(kc) != nk or len(kb) != nk or len(frames) != nk:
            raise OrbxError(-1, f"{who}: {nk} keyframe slots need centre [{nk}][3], bad [{nk}] and {nk} frames")
        fr = (C.c_void_p * max(nk, 1))(*[None if f is None else f._h for f in frames])
        ts = None if table_slots is None else MapPoints._slots(table_slots)
        po = None if pos is None else np.ascontiguousarray(pos, np.float32)
        rk = None if ref_kf is None else np.ascontiguousarray(ref_kf, np.int32).reshape(-1)
        sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        if (ts is not None and len(ts) != n) or (po is not None and po.shape != (n, 3)) or (rk is not None and len(rk) != n):
            raise OrbxError(-1, f"{who}: {n} points need table_slots [{n}], pos [{n}][3] and ref_kf [{n}]")
        job = RefreshJob(int(what), n, _p(pt), None if ts is None else _p(ts), None if po is None else _p(po), None if rk is None else _p(rk),
                         nk, _p(ks), _p(kc), _p(kb), fr, None if sf is None else _p(sf), 0 if sf is None else len(sf))
        r = RefreshResult(n) if out is None else out
        if any(len(a) != n for a in (r.status, r.geom, r.best_kf, r.best_idx, r.desc)):
            raise OrbxError(-1, f"{who}: out holds {len(r.status)} rows, {n} points are listed")
        _check(lib().orbx_mapgraph_refresh_points(self._h, None if table is None else table._h, C.byref(job), _p(r.status), _p(r.geom),
                                                  _p(r.best_kf), _p(r.best_idx), _p(r.desc), stream))
        return r


def _pose_inputs(cam, Tcw, who):
    ca = np.ascontiguousarray(cam, np.float32).reshape(-1); tc = np.ascontiguousarray(Tcw, np.float32).reshape(-1)
    if len(ca) != 5 or len(tc) != 16:
        raise OrbxError(-1, f"{who}: cam is fx fy cx cy mbf, Tcw is 4 x 4")
    return ca, tc


def _pose_result(Tcw_out, outlier, n_inliers, rep):
    return dict(Tcw=Tcw_out.reshape(4, 4), outlier=outlier, n_inliers=n_inliers, n_corr=rep.n_corr, rounds=rep.rounds,
                n_bad=np.array(rep.n_bad[:], np.int32), iterations=np.array(rep.iterations[:], np.int32),
                chi2=np.array(rep.chi2[:], np.float64), pose=np.array(rep.pose[:], np.float64).reshape(3, 4))


def _pose_obs(obs, who):
    """obs = dict(x, y, u_right, inv_sigma2, Xw[n][3], has_point) -> (PoseObs, the arrays it points into)"""
    keep = [np.ascontiguousarray(obs[k], np.float32) for k in ("x", "y", "u_right", "inv_sigma2")]
    n = len(keep[0])
    keep.append(np.ascontiguousarray(obs["Xw"], np.float32).reshape(-1, 3))
    keep.append(np.ascontiguousarray(obs["has_point"], np.uint8))
    if any(a.ndim != 1 or len(a) != n for a in keep[:4]) or keep[4].shape != (n, 3) or keep[5].shape != (n,):
        raise OrbxError(-1, f"{who}: x, y, u_right, inv_sigma2, has_point need n entries, Xw [n][3]")
    return PoseObs(n, *[_p(a) for a in keep]), keep


def pose_optimize(obs, cam, Tcw, device=0):
    """Optimizer::PoseOptimization (orbx_pose_optimize): obs = dict(x, y, u_right, inv_sigma2, Xw, has_point), cam = fx fy cx cy mbf,
    Tcw 4 x 4 -> dict(Tcw, outlier, n_inliers, n_corr, rounds, n_bad, iterations, chi2, pose)"""
    po, keep = _pose_obs(obs, "pose_optimize")
    ca, tc = _pose_inputs(cam, Tcw, "pose_optimize")
    out = np.zeros(16, np.float32); fl = np.zeros(po.n, np.uint8); ni = C.c_int(); rep = PoseReport()
    _check(lib().orbx_pose_optimize(device, C.byref(po), _p(ca), _p(tc), _p(out), _p(fl), C.byref(ni), C.byref(rep)))
    return _pose_result(out, fl, ni.value, rep)


def _lba_problem(problem, who):
    """problem = dict(Tcw [K][4][4], cam [K][5], fixed [K], Xw [P][3], edge_kf, edge_point, x, y, u_right, inv_sigma2) -> (LbaProblem, arrays)"""
    Tcw = np.ascontiguousarray(problem["Tcw"], np.float32).reshape(-1, 16)
    K = len(Tcw)
    cam = np.ascontiguousarray(problem["cam"], np.float32).reshape(-1, 5)
    fixed = np.ascontiguousarray(problem["fixed"], np.uint8).reshape(-1)
    Xw = np.ascontiguousarray(problem["Xw"], np.float32).reshape(-1, 3)
    ek = np.ascontiguousarray(problem["edge_kf"], np.int32).reshape(-1)
    ep = np.ascontiguousarray(problem["edge_point"], np.int32).reshape(-1)
    obs = [np.ascontiguousarray(problem[k], np.float32).reshape(-1) for k in ("x", "y", "u_right", "inv_sigma2")]
    if len(cam) != K or len(fixed) != K or any(len(a) != len(ek) for a in [ep] + obs):
        raise OrbxError(-1, f"{who}: Tcw, cam and fixed need one entry per keyframe, the edge arrays one per edge")
    keep = [Tcw, cam, fixed, Xw, ek, ep] + obs
    return LbaProblem(K, _p(Tcw), _p(cam), _p(fixed), len(Xw), _p(Xw), len(ek), _p(ek), _p(ep), *[_p(a) for a in obs]), keep


def local_bundle_adjustment(problem, stop_at_trial=-1, stop=None, device=0):
    """Optimizer::LocalBundleAdjustment (orbx_local_bundle_adjustment): problem = dict(Tcw [K][4][4], cam [K][5] fx fy cx cy mbf, fixed [K],
    Xw [P][3], edge_kf, edge_point, x, y, u_right, inv_sigma2 [E]); stop: a uint8 array of one element that is polled as mbAbortBA;
    stop_at_trial: the debug_stop_at_trial hook -> dict(Tcw [K][4][4], Xw [P][3], edge_flags [E], pose [K][3][4], point [P][3], stopped,
    iterations, trials, n_level1, n_erase, n_active_kf, n_active_points, chi2, lambda)"""
    pr, keep = _lba_problem(problem, "local_bundle_adjustment")
    opt = LbaOptions(stop.ctypes.data if stop is not None else None, int(stop_at_trial))
    Tcw = np.zeros((pr.n_kf, 4, 4), np.float32); Xw = np.zeros((pr.n_points, 3), np.float32); fl = np.zeros(pr.n_edges, np.uint8)
    pose = np.zeros((pr.n_kf, 3, 4), np.float64); point = np.zeros((pr.n_points, 3), np.float64); rep = LbaReport()
    _check(lib().orbx_local_bundle_adjustment(device, C.byref(pr), C.byref(opt), _p(Tcw), _p(Xw), _p(fl), _p(pose), _p(point), C.byref(rep)))
    return {"Tcw": Tcw, "Xw": Xw, "edge_flags": fl, "pose": pose, "point": point, "stopped": rep.stopped, "iterations": list(rep.iterations),
            "trials": list(rep.trials), "n_level1": rep.n_level1, "n_erase": rep.n_erase, "n_active_kf": list(rep.n_active_kf),
            "n_active_points": list(rep.n_active_points), "chi2": list(rep.chi2), "lambda": list(rep.lambda_)}


def bundle_adjustment(problem, iterations=10, robust=True, stop=None, stop_at_trial=-1, device=0):
    """Optimizer::BundleAdjustment (orbx_bundle_adjustment): problem as for local_bundle_adjustment; iterations: 20 at map creation, 10
    after a loop; stop: a uint8 array of one element polled as pbStopFlag; stop_at_trial: the debug_stop_at_trial hook -> dict(Tcw
    [K][4][4], Xw [P][3], point_included [P], pose [K][3][4], point [P][3], stopped, iterations, trials, n_active_kf, n_active_points, chi2,
    lambda, lambda_init)"""
    pr, keep = _lba_problem(problem, "bundle_adjustment")
    opt = BaOptions(stop.ctypes.data if stop is not None else None, int(stop_at_trial), int(iterations), int(bool(robust)))
    Tcw = np.zeros((pr.n_kf, 4, 4), np.float32); Xw = np.zeros((pr.n_points, 3), np.float32); inc = np.zeros(pr.n_points, np.uint8)
    pose = np.zeros((pr.n_kf, 3, 4), np.float64); point = np.zeros((pr.n_points, 3), np.float64); rep = BaReport()
    _check(lib().orbx_bundle_adjustment(device, C.byref(pr), C.byref(opt), _p(Tcw), _p(Xw), _p(inc), _p(pose), _p(point), C.byref(rep)))
    return {"Tcw": Tcw, "Xw": Xw, "point_included": inc, "pose": pose, "point": point, "stopped": rep.stopped, "iterations": rep.iterations,
            "trials": rep.trials, "n_active_kf": rep.n_active_kf, "n_active_points": rep.n_active_points, "chi2": rep.chi2,
            "lambda": rep.lambda_, "lambda_init": rep.lambda_init}


def _eg_problem(problem, who):
    """problem = dict(Tcw [K][4][4], fixed [K], corrected [K], noncorrected [K], S_corrected [.][8], S_noncorrected [.][8], edge_i, edge_j,
    edge_kind [E], Xw [P][3], point_ref [P], fix_scale) -> (EgProblem, arrays)"""
    Tcw = np.ascontiguousarray(problem["Tcw"], np.float32).reshape(-1, 16)
    K = len(Tcw)
    fixed = np.ascontiguousarray(problem["fixed"], np.uint8).reshape(-1)
    cor = np.ascontiguousarray(problem["corrected"], np.int32).reshape(-1)
    non = np.ascontiguousarray(problem["noncorrected"], np.int32).reshape(-1)
    Sc = np.ascontiguousarray(problem["S_corrected"], np.float64).reshape(-1, 8)
    Sn = np.ascontiguousarray(problem["S_noncorrected"], np.float64).reshape(-1, 8)
    ei = np.ascontiguousarray(problem["edge_i"], np.int32).reshape(-1)
    ej = np.ascontiguousarray(problem["edge_j"], np.int32).reshape(-1)
    kind = np.ascontiguousarray(problem["edge_kind"], np.uint8).reshape(-1)
    Xw = np.ascontiguousarray(problem["Xw"], np.float32).reshape(-1, 3)
    ref = np.ascontiguousarray(problem["point_ref"], np.int32).reshape(-1)
    if len(fixed) != K or len(cor) != K or len(non) != K or len(ej) != len(ei) or len(kind) != len(ei) or len(ref) != len(Xw):
        raise OrbxError(-1, f"{who}: Tcw, fixed, corrected and noncorrected need one entry per keyframe, the edge arrays one per edge, point_ref one per point")
    keep = [Tcw, fixed, cor, non, Sc, Sn, ei, ej, kind, Xw, ref]
    return EgProblem(K, _p(Tcw), _p(fixed), _p(cor), _p(non), len(Sc), len(Sn), _p(Sc), _p(Sn), len(ei), _p(ei), _p(ej), _p(kind), len(Xw), _p(Xw),
                     _p(ref), int(bool(problem["fix_scale"]))), keep


def optimize_essential_graph(problem, iterations=20, device=0, solver=None):
    """Optimizer::OptimizeEssentialGraph (orbx_optimize_essential_graph): problem = dict(Tcw [K][4][4], fixed [K] (exactly one set: pLoopKF),
    corrected / noncorrected [K] (index into S_corrected / S_noncorrected [.][8] qx qy qz qw tx ty tz s, or -1), edge_i, edge_j, edge_kind [E]
    (0 loop-connection edge, 1 normal edge), Xw [P][3], point_ref [P], fix_scale) -> dict(Tcw [K][4][4], Xw [P][3], S [K][8], point [P][3],
    iterations, trials, n_free, n_solve_failed, chi2_start, chi2, lambda).  solver: None is orbx_optimize_essential_graph (the dense solve, up
    to 1536 free keyframes); EG_SOLVER_DENSE, EG_SOLVER_ENVELOPE or EG_SOLVER_AUTO goes to orbx_optimize_essential_graph2 (ENVELOPE and AUTO:
    up to 4095 free keyframes, the same values as the dense solve)"""
    pr, keep = _eg_problem(problem, "optimize_essential_graph")
    Tcw = np.zeros((pr.n_kf, 4, 4), np.float32); Xw = np.zeros((pr.n_points, 3), np.float32)
    S = np.zeros((pr.n_kf, 8), np.float64); point = np.zeros((pr.n_points, 3), np.float64); rep = EgReport()
    if solver is None:
        opt = EgOptions(int(iterations))
        _check(lib().orbx_optimize_essential_graph(device, C.byref(pr), C.byref(opt), _p(Tcw), _p(Xw), _p(S), _p(point), C.byref(rep)))
    else:
        opt = EgOptions2(int(iterations), int(solver))
        _check(lib().orbx_optimize_essential_graph2(device, C.byref(pr), C.byref(opt), _p(Tcw), _p(Xw), _p(S), _p(point), C.byref(rep)))
    return {"Tcw": Tcw, "Xw": Xw, "S": S, "point": point, "iterations": rep.iterations, "trials": rep.trials, "n_free": rep.n_free,
            "n_solve_failed": rep.n_solve_failed, "chi2_start": rep.chi2_start, "chi2": rep.chi2, "lambda": rep.lambda_}


def eg_envelope(problem):
    """orbx_eg_envelope: what the problem's keyframe order costs the envelope solve -> (entries, triangle): the doubles of the envelope of
    the 7 F x 7 F system and of its whole lower triangle.  Host only: no device is opened."""
    pr, keep = _eg_problem(problem, "eg_envelope")
    entries, triangle = C.c_int64(-1), C.c_int64(-1)
    _check(lib().orbx_eg_envelope(C.byref(pr), C.byref(entries), C.byref(triangle)))
    return int(entries.value), int(triangle.value)


EG_STAGES = ("vS", "meas", "xf", "rec", "echi", "Hd", "bv", "pair", "Off", "status_lin", "err", "S", "y", "solve_ok", "x", "trial", "sc",
             "echi_trial", "status_trial")
EG_STAGES_MAX_N, EG_STAGES_MAX_PROBED = 1024, 4096


def eg_stages(problem, lam, x=None, trial=True, want=None, device=0):
    """orbx_debug_eg_stages: one linearisation of the essential graph at its start estimates and, with trial, one Levenberg trial with
    lambda = lam, through the launch sequences of optimize_essential_graph; x [7 F]: the solve is skipped and the update reads x.
    want: names of EG_STAGES (default all but "S" and "err"; without trial, those of the linearisation) -> dict of the arrays as
    include/orbx.h lays them out: vS, trial [K][8], meas [E][8], xf [14][8], rec [E][120], echi, echi_trial [E], Hd [F][28], bv [F][7],
    pair [NP][2] (with n_pairs), Off [NP][49], status_lin, status_trial [4], err [E][29][7], S [n][n], y, x [n], sc [F], solve_ok"""
    pr, keep = _eg_problem(problem, "eg_stages")
    K, E, F = pr.n_kf, pr.n_edges, pr.n_kf - 1
    n = 7 * F
    want = [k for k in EG_STAGES if k not in ("S", "err")] if want is None else list(want)
    for k in want:
        if k not in EG_STAGES:
            raise OrbxError(-1, f"eg_stages: no stage {k!r}")
    ran = E > 0 and F > 0
    if not trial or not ran:
        want = [k for k in want if k not in EG_STAGES[11:]]
    if not ran:
        want = [k for k in want if k in ("vS", "meas", "xf", "pair")]
    shapes = dict(vS=(K, 8), meas=(E, 8), xf=(14, 8), rec=(E, 120), echi=(E,), Hd=(F, 28), bv=(F, 7), pair=(E, 2), Off=(E, 49), status_lin=(4,),
                  err=(E, 29, 7), S=(n, n), y=(n,), solve_ok=(1,), x=(n,), trial=(K, 8), sc=(F,), echi_trial=(E,), status_trial=(4,))
    out = {k: np.zeros(shapes[k], np.int32 if k in ("pair", "solve_ok") else np.float64) for k in want}
    if "Off" in out and "pair" not in out:
        out["pair"] = np.zeros(shapes["pair"], np.int32)
    npairs = np.zeros(1, np.int32)
    d = EgStages(**{k: _p(v) for k, v in out.items()}, n_pairs=_p(npairs))
    xin = None if x is None else np.ascontiguousarray(x, np.float64).reshape(-1)
    if xin is not None and len(xin) != n:
        raise OrbxError(-1, f"eg_stages: x has {len(xin)} entries, not 7 x {F}")
    _check(lib().orbx_debug_eg_stages(device, C.byref(pr), float(lam), None if xin is None else _p(xin), int(bool(trial)), C.byref(d)))
    NP = int(npairs[0])
    for k in ("pair", "Off"):
        if k in out:
            out[k] = out[k][:NP].copy()
    if "solve_ok" in out:
        out["solve_ok"] = int(out["solve_ok"][0])
    out["n_pairs"] = NP
    return out


def ldlt_solve(S, b, form, x0=None, device=0):
    """orbx_debug_ldlt_solve: the dense LDL^T of the bundle adjustments on S x = b (S [n][n], its lower triangle read), form 0 = one
    workgroup (n <= 1536), 1 = panels -> (x [n], ok); after a pivot that is not > 0, ok is False and x is x0 (zeros) untouched"""
    S = np.ascontiguousarray(S, np.float64); b = np.ascontiguousarray(b, np.float64).reshape(-1)
    n = len(b)
    if S.shape != (n, n):
        raise OrbxError(-1, "ldlt_solve: S must be [n][n] for b [n]")
    x = np.zeros(n) if x0 is None else np.array(x0, np.float64).reshape(n)
    ok = C.c_int(-1)
    _check(lib().orbx_debug_ldlt_solve(device, n, _p(S), _p(b), _p(x), int(form), C.byref(ok)))
    return x, bool(ok.value)


def ldlt_solve_envelope(S, b, first, x0=None, device=0):
    """orbx_debug_ldlt_solve_envelope: the envelope form of the panel LDL^T on S x = b.  S [n][n] dense, first [n] every row's first column
    (0 <= first[i] <= i, rounded down to the panel width by the library): only the entries first[i] <= j <= i are read -> (x [n], ok) as
    ldlt_solve"""
    S = np.ascontiguousarray(S, np.float64); b = np.ascontiguousarray(b, np.float64).reshape(-1)
    first = np.ascontiguousarray(first, np.int32).reshape(-1)
    n = len(b)
    if S.shape != (n, n) or len(first) != n:
        raise OrbxError(-1, "ldlt_solve_envelope: S must be [n][n] and first [n] for b [n]")
    x = np.zeros(n) if x0 is None else np.array(x0, np.float64).reshape(n)
    ok = C.c_int(-1)
    _check(lib().orbx_debug_ldlt_solve_envelope(device, n, _p(first), _p(S), _p(b), _p(x), C.byref(ok)))
    return x, bool(ok.value)


def ldlt_panel_width():
    """the panel width of form 1 of the dense LDL^T (orbx_debug_ldlt_panel_width)"""
    return lib().orbx_debug_ldlt_panel_width()


def set_lba_solver(form):
    """orbx_debug_set_lba_solver: the calling thread's later local_bundle_adjustment calls solve with form 0 (one workgroup, the default)
    or 1 (panels)"""
    _check(lib().orbx_debug_set_lba_solver(int(form)))


def pose_optimize_batch(jobs, device=0):
    """orbx_pose_optimize_batch: jobs = [(obs, cam, Tcw), ...] in one upload, one launch, one download -> [dict as pose_optimize]"""
    nj = len(jobs)
    arr = (PoseJob * max(nj, 1))()
    keep = []
    for j, (obs, cam, Tcw) in enumerate(jobs):
        po, k = _pose_obs(obs, "pose_optimize_batch")
        ca, tc = _pose_inputs(cam, Tcw, "pose_optimize_batch")
        out = np.zeros(16, np.float32); fl = np.zeros(po.n, np.uint8); rep = PoseReport()
        keep.append((po, k, ca, tc, out, fl, rep))
        arr[j].obs = C.pointer(po); arr[j].cam = _p(ca); arr[j].Tcw = _p(tc); arr[j].Tcw_out = _p(out); arr[j].outlier = _p(fl)
        arr[j].report = C.pointer(rep)
    _check(lib().orbx_pose_optimize_batch(device, arr, nj))
    return [_pose_result(k[4], k[5], arr[j].n_inliers, k[6]) for j, k in enumerate(keep)]


SIM3OPT_FIELDS = ("x1", "y1", "inv_sigma2_1", "x2", "y2", "inv_sigma2_2")


def sim3opt_camera_points(Xw, Rcw, tcw):
    """the camera-frame points Optimizer::OptimizeSim3 hands g2o (src/Optimizer.cc:1241-1251: `R1w*P3D1w + t1w` on CV_32F matrices), by the
    rule of include/orbx.h for cv::Mat products: (float)dotd(R.row(r), Xw) -- double products, double sum, one cast -- then the float add
    of t[r].  Xw [n][3], Rcw 3 x 3, tcw [3], all float32 -> [n][3] float32"""
    X = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3).astype(np.float64)
    R = np.ascontiguousarray(Rcw, np.float32).reshape(3, 3).astype(np.float64)
    t = np.ascontiguousarray(tcw, np.float32).reshape(3)
    P = ((X[:, None, 0] * R[None, :, 0] + X[:, None, 1] * R[None, :, 1]) + X[:, None, 2] * R[None, :, 2]).astype(np.float32)
    return P + t[None, :]


def _sim3opt_obs(obs, who):
    """obs = dict(has_pair, P1c[n][3], P2c[n][3], x1, y1, inv_sigma2_1, x2, y2, inv_sigma2_2) -> (Sim3OptObs, the arrays it points into)"""
    keep = [np.ascontiguousarray(obs["has_pair"], np.uint8)]
    n = len(keep[0])
    keep += [np.ascontiguousarray(obs[k], np.float32).reshape(-1, 3) for k in ("P1c", "P2c")]
    keep += [np.ascontiguousarray(obs[k], np.float32) for k in SIM3OPT_FIELDS]
    if keep[0].ndim != 1 or any(a.shape != (n, 3) for a in keep[1:3]) or any(a.shape != (n,) for a in keep[3:]):
        raise OrbxError(-1, f"{who}: has_pair, x1, y1, inv_sigma2_1, x2, y2, inv_sigma2_2 need n entries, P1c and P2c [n][3]")
    return Sim3OptObs(n, *[_p(a) for a in keep]), keep


def _sim3opt_inputs(cam1, cam2, S12, who):
    c1 = np.ascontiguousarray(cam1, np.float32).reshape(-1); c2 = np.ascontiguousarray(cam2, np.float32).reshape(-1)
    s = np.ascontiguousarray(S12, np.float64).reshape(-1)
    if len(c1) != 4 or len(c2) != 4 or len(s) != 8:
        raise OrbxError(-1, f"{who}: cam1 and cam2 are fx fy cx cy, S12 is qx qy qz qw tx ty tz s")
    return c1, c2, s


def _sim3opt_result(S12_out, inlier, n_inliers, rep):
    return dict(S12=S12_out, inlier=inlier, n_inliers=n_inliers, n_corr=rep.n_corr, rounds=rep.rounds, n_bad=rep.n_bad,
                more_iterations=rep.more_iterations, iterations=np.array(rep.iterations[:], np.int32),
                chi2=np.array(rep.chi2[:], np.float64), report_S12=np.array(rep.S12[:], np.float64))


def sim3_optimize(obs, cam1, cam2, S12, th2, fix_scale, device=0):
    """Optimizer::OptimizeSim3 (orbx_sim3_optimize): obs = dict(has_pair, P1c, P2c, x1, y1, inv_sigma2_1, x2, y2, inv_sigma2_2), cam =
    fx fy cx cy, S12 = qx qy qz qw tx ty tz s -> dict(S12, inlier, n_inliers, n_corr, rounds, n_bad, more_iterations, iterations, chi2,
    report_S12)"""
    so, keep = _sim3opt_obs(obs, "sim3_optimize")
    c1, c2, s = _sim3opt_inputs(cam1, cam2, S12, "sim3_optimize")
    out = np.zeros(8, np.float64); fl = np.zeros(so.n, np.uint8); ni = C.c_int(); rep = Sim3OptReport()
    _check(lib().orbx_sim3_optimize(device, C.byref(so), _p(c1), _p(c2), _p(s), float(th2), int(bool(fix_scale)), _p(out), _p(fl), C.byref(ni),
                                    C.byref(rep)))
    return _sim3opt_result(out, fl, ni.value, rep)


def sim3_optimize_batch(jobs, device=0):
    """orbx_sim3_optimize_batch: jobs = [(obs, cam1, cam2, S12, th2, fix_scale), ...] in one upload, one launch, one download
    -> [dict as sim3_optimize]"""
    nj = len(jobs)
    arr = (Sim3OptJob * max(nj, 1))()
    keep = []
    for j, (obs, cam1, cam2, S12, th2, fix_scale) in enumerate(jobs):
        so, k = _sim3opt_obs(obs, "sim3_optimize_batch")
        c1, c2, s = _sim3opt_inputs(cam1, cam2, S12, "sim3_optimize_batch")
        out = np.zeros(8, np.float64); fl = np.zeros(so.n, np.uint8); rep = Sim3OptReport()
        keep.append((so, k, c1, c2, s, out, fl, rep))
        arr[j].obs = C.pointer(so); arr[j].cam1 = _p(c1); arr[j].cam2 = _p(c2); arr[j].S12 = _p(s); arr[j].th2 = float(th2)
        arr[j].fix_scale = int(bool(fix_scale)); arr[j].S12_out = _p(out); arr[j].inlier = _p(fl); arr[j].report = C.pointer(rep)
    _check(lib().orbx_sim3_optimize_batch(device, arr, nj))
    return [_sim3opt_result(k[5], k[6], arr[j].n_inliers, k[7]) for j, k in enumerate(keep)]


def _tri_view(v, who):
    """dict(Tcw 3 x 4 (or 4 x 4: the top rows), Ow[3], fx, fy, cx, cy, invfx, invfy, mb, mbf) -> TriView"""
    T = np.ascontiguousarray(v["Tcw"], np.float32).reshape(-1)
    ow = np.ascontiguousarray(v["Ow"], np.float32).reshape(-1)
    if len(T) not in (12, 16) or len(ow) != 3:
        raise OrbxError(-1, f"{who}: a view needs Tcw 3 x 4 (or 4 x 4) and Ow[3]")
    return TriView((C.c_float * 12)(*T[:12]), (C.c_float * 3)(*ow), *[float(v[k]) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")])


def _tri_feats(k, who):
    """dict(x, y, octave, u_right[, depth, raw_x, raw_y]) -> (TriFeats, the arrays it points into)"""
    keep = [np.ascontiguousarray(k["x"], np.float32), np.ascontiguousarray(k["y"], np.float32), np.ascontiguousarray(k["octave"], np.int32),
            np.ascontiguousarray(k["u_right"], np.float32)]
    n = len(keep[0])
    for name in ("depth", "raw_x", "raw_y"):
        a = k.get(name)
        keep.append(None if a is None else np.ascontiguousarray(a, np.float32))
    if any(a is not None and (a.ndim != 1 or len(a) != n) for a in keep):
        raise OrbxError(-1, f"{who}: the arrays of a keyframe need one entry per feature")
    return TriFeats(n, *[_p(a) for a in keep]), keep


def _tri_lists(n2, pairs, npairs, scaleFactors, levelSigma2, who):
    """pairs [n2][2*cap] (or [n2][cap][2]) int32 and npairs[n2] as SearchForTriangulationBatch's ABI call returns them"""
    pr = np.ascontiguousarray(pairs, np.int32)
    npr = np.ascontiguousarray(npairs, np.int32).reshape(-1)
    if pr.size == 0 or len(npr) != n2 or n2 == 0 or pr.size % (2 * n2):
        raise OrbxError(-1, f"{who}: pairs is [n2][2*cap] with cap >= 1 and npairs [n2], n2 = {n2} keyframes >= 1")
    sf = np.ascontiguousarray(scaleFactors, np.float32).reshape(-1); sg = np.ascontiguousarray(levelSigma2, np.float32).reshape(-1)
    if len(sf) != len(sg):
        raise OrbxError(-1, f"{who}: scaleFactors and levelSigma2 are one table of levels each")
    cap = pr.size // (2 * n2)
    return pr, npr, cap, sf, sg, np.zeros((n2, cap), np.uint8), np.zeros((n2, cap, 3), np.float32)


def triangulate_pairs(k1, v1, k2s, v2s, pairs, npairs, scaleFactors, levelSigma2, ratioFactor, device=0):
    """The match loop body of LocalMapping::CreateNewMapPoints (orbx_triangulate_pairs): k1 / k2s[i] = dict(x, y, octave, u_right[, depth,
    raw_x, raw_y]), v1 / v2s[i] = dict(Tcw, Ow, fx, fy, cx, cy, invfx, invfy, mb, mbf), pairs[n2][2*cap], npairs[n2]
    -> (status[n2][cap], x3d[n2][cap][3], n_new); rows are written up to npairs[i]"""
    who = "triangulate_pairs"
    n2 = len(k2s)
    if len(v2s) != n2:
        raise OrbxError(-1, f"{who}: {n2} keyframes, {len(v2s)} views")
    pr, npr, cap, sf, sg, status, x3d = _tri_lists(n2, pairs, npairs, scaleFactors, levelSigma2, who)
    f1, keep1 = _tri_feats(k1, who)
    fs = [_tri_feats(k, who) for k in k2s]
    ptrs = (C.POINTER(TriFeats) * n2)(*[C.pointer(f[0]) for f in fs])
    views = (TriView * n2)(*[_tri_view(v, who) for v in v2s])
    n_new = C.c_int()
    _check(lib().orbx_triangulate_pairs(device, C.byref(f1), C.byref(_tri_view(v1, who)), ptrs, views, n2, _p(pr), cap, _p(npr), _p(sf), _p(sg),
                                        len(sf), float(ratioFactor), _p(status), _p(x3d), C.byref(n_new)))
    return status, x3d, n_new.value


def frame_set_depth(frame, depth, raw_x=None, raw_y=None):
    """orbx_frame_set_depth: mvDepth and, where they differ from the undistorted ones, the raw positions of a DeviceFrame; once per frame"""
    arrs = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1) for a in (depth, raw_x, raw_y)]
    if any(a is not None and len(a) != frame.n for a in arrs):
        raise OrbxError(-1, f"frame_set_depth: the frame has {frame.n} features")
    _check(lib().orbx_frame_set_depth(frame._h, *[_p(a) for a in arrs]))


def frame_triangulate(k1, v1, k2s, v2s, pairs, npairs, scaleFactors, levelSigma2, ratioFactor):
    """triangulate_pairs on DeviceFrames (orbx_frame_triangulate): only the views and the pair lists go up"""
    who = "frame_triangulate"
    n2 = len(k2s)
    if len(v2s) != n2:
        raise OrbxError(-1, f"{who}: {n2} keyframes, {len(v2s)} views")
    pr, npr, cap, sf, sg, status, x3d = _tri_lists(n2, pairs, npairs, scaleFactors, levelSigma2, who)
    hs = (C.c_void_p * n2)(*[k._h for k in k2s])
    views = (TriView * n2)(*[_tri_view(v, who) for v in v2s])
    n_new = C.c_int()
    _check(lib().orbx_frame_triangulate(k1._h, C.byref(_tri_view(v1, who)), hs, views, n2, _p(pr), cap, _p(npr), _p(sf), _p(sg), len(sf),
                                        float(ratioFactor), _p(status), _p(x3d), C.byref(n_new)))
    return status, x3d, n_new.value


def _sim3_job(job, who):
    """dict(X1[n][3], X2[n][3], max_err1[n], max_err2[n], K1[4], K2[4], fix_scale, samples[n_hyp][3]) -> (Sim3Job, inputs, outputs)"""
    X1, X2 = np.ascontiguousarray(job["X1"], np.float32), np.ascontiguousarray(job["X2"], np.float32)
    e1, e2 = np.ascontiguousarray(job["max_err1"], np.float32).reshape(-1), np.ascontiguousarray(job["max_err2"], np.float32).reshape(-1)
    sa = np.ascontiguousarray(job["samples"], np.int32)
    k1, k2 = np.asarray(job["K1"], np.float32).reshape(-1), np.asarray(job["K2"], np.float32).reshape(-1)
    n = len(X1)
    if X1.shape != (n, 3) or X2.shape != (n, 3) or len(e1) != n or len(e2) != n or sa.ndim != 2 or sa.shape[1] != 3 or len(k1) != 4 or len(k2) != 4:
        raise OrbxError(-1, f"{who}: X1, X2 [n][3], max_err1, max_err2 [n], samples [n_hyp][3], K1, K2 [4]")
    nh = len(sa)
    out = (np.zeros(nh, np.int32), np.zeros((nh, 13), np.float32), np.zeros((nh, (n + 63) // 64), np.uint64))
    J = Sim3Job(n, _p(X1), _p(X2), _p(e1), _p(e2), (C.c_float * 4)(*k1), (C.c_float * 4)(*k2), int(bool(job["fix_scale"])), nh, _p(sa),
                *[_p(a) for a in out])
    return J, (X1, X2, e1, e2, sa), out


def sim3_hypotheses(job, device=0):
    """Sim3Solver's ComputeSim3 + CheckInliers for every sample row of one solver (orbx_sim3_hypotheses): job = dict(X1, X2, max_err1,
    max_err2, K1, K2, fix_scale, samples) -> (n_inliers[n_hyp] int32, srt[n_hyp][13] float32, inlier_bits[n_hyp][(n+63)/64] uint64)"""
    J, keep, out = _sim3_job(job, "sim3_hypotheses")
    _check(lib().orbx_sim3_hypotheses(device, C.byref(J)))
    return out


def sim3_hypotheses_batch(jobs, device=0):
    """orbx_sim3_hypotheses_batch: the solvers of one ComputeSim3 call in one upload, one launch, one download -> [as sim3_hypotheses]"""
    nj = len(jobs)
    arr = (Sim3Job * max(nj, 1))()
    keep = []
    for j, job in enumerate(jobs):
        J, k, out = _sim3_job(job, "sim3_hypotheses_batch")
        arr[j] = J
        keep.append((J, k, out))
    _check(lib().orbx_sim3_hypotheses_batch(device, arr, nj))
    return [k[2] for k in keep]


def sim3_max_error(sigma2):
    """mvnMaxError1/2 (reference include/Sim3Solver.h:78-79 keeps 9.210 * sigma2 in a vector<size_t>): the float the comparison sees"""
    return np.float32(int(9.210 * float(np.float32(sigma2))))


class Sim3Ransac:
    """Sim3Solver's RANSAC state machine (reference src/Sim3Solver.cc:117-217) over a table of hypotheses: the first iterate() or find()
    evaluates every row of `samples` (at least mRansacMaxIts of them) on the device, in one call, and every call replays the reference's
    loop over the table.  job as sim3_hypotheses; indices1 = mvnIndices1 and n_matches = mN1 scatter the inliers as the reference does.
    sim3_hypotheses_batch([r.job for r in solvers]) + r.set_table(...) evaluates several solvers in one launch."""

    def __init__(self, job, indices1=None, n_matches=None, probability=0.99, min_inliers=6, max_iterations=300, device=0):
        self.job, self.device = job, device
        self.N = len(job["X1"])
        self.indices1 = np.arange(self.N) if indices1 is None else np.asarray(indices1, np.int64)
        self.mN1 = self.N if n_matches is None else int(n_matches)
        self.table = None
        self.best_inliers, self.best = 0, None
        self.set_ransac_parameters(probability, min_inliers, max_iterations)

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        import math
        self.min_inliers = min_inliers
        n_it = 1
        if min_inliers != self.N:
            with np.errstate(all="ignore"):
                eps = np.float32(min_inliers) / np.float32(self.N)
                x = np.log(np.float64(1.0) - np.float64(probability)) / np.log(np.float64(1.0) - np.float64(eps) ** 3)
            n_it = int(math.ceil(float(x))) if np.isfinite(x) else -2 ** 31
        self.max_its = max(1, min(n_it, max_iterations))
        self.iterations = 0
        self.table = None

    def set_table(self, table):
        self.table = table

    def _row(self, k):
        ni, srt, bits = self.table
        inl = np.unpackbits(np.ascontiguousarray(bits[k], "<u8").view(np.uint8), bitorder="little")[:self.N].astype(bool)
        return int(ni[k]), srt[k], inl

    def iterate(self, n_iterations):
        """-> (T12 4 x 4 float32 or None, bNoMore, vbInliers[mN1], nInliers)"""
        vb = np.zeros(self.mN1, bool)
        if self.N < self.min_inliers:
            return None, True, vb, 0
        if self.table is None:
            if len(self.job["samples"]) < self.max_its:
                raise OrbxError(-1, f"Sim3Ransac: {len(self.job['samples'])} sample rows for {self.max_its} iterations")
            self.table = sim3_hypotheses(dict(self.job, samples=np.asarray(self.job["samples"])[:self.max_its]), self.device)
        cur = 0
        while self.iterations < self.max_its and cur < n_iterations:
            cur += 1
            self.iterations += 1
            ni, srt, inl = self._row(self.iterations - 1)
            if ni >= self.best_inliers:
                self.best_inliers, self.best = ni, (srt.copy(), inl)
                if ni > self.min_inliers:
                    vb[self.indices1[inl]] = True
                    return self.T12(srt), False, vb, ni
        return None, self.iterations >= self.max_its, vb, 0

    def find(self):
        T, _, vb, ni = self.iterate(self.max_its)
        return T, vb, ni

    @staticmethod
    def T12(srt):
        T = np.eye(4, dtype=np.float32)
        with np.errstate(all="ignore"):
            T[:3, :3] = (np.float64(srt[0]) * srt[1:10].astype(np.float64)).astype(np.float32).reshape(3, 3)
        T[:3, 3] = srt[10:13]
        return T

    def estimated_scale(self):
        return self.best[0][0]

    def estimated_rotation(self):
        return self.best[0][1:10].reshape(3, 3).copy()

    def estimated_translation(self):
        return self.best[0][10:13].copy()


def _pnp_job(job, who):
    """dict(P3Dw[n][3], P2D[n][2], max_err[n], K[4] = fu fv uc vc, min_inliers, samples[n_hyp][4]) -> (PnpJob, inputs, outputs)"""
    P3, P2 = np.ascontiguousarray(job["P3Dw"], np.float32), np.ascontiguousarray(job["P2D"], np.float32)
    me = np.ascontiguousarray(job["max_err"], np.float32).reshape(-1)
    sa = np.ascontiguousarray(job["samples"], np.int32)
    k = np.asarray(job["K"], np.float64).reshape(-1)
    n = len(P3)
    if P3.shape != (n, 3) or P2.shape != (n, 2) or len(me) != n or sa.ndim != 2 or sa.shape[1] != 4 or len(k) != 4:
        raise OrbxError(-1, f"{who}: P3Dw [n][3], P2D [n][2], max_err [n], samples [n_hyp][4], K [4]")
    nh, words = len(sa), (n + 63) // 64
    out = (np.zeros(nh, np.int32), np.zeros((nh, 12), np.float64), np.zeros((nh, words), np.uint64),
           np.zeros(nh, np.int32), np.zeros((nh, 12), np.float64), np.zeros((nh, words), np.uint64))
    J = PnpJob(n, _p(P3), _p(P2), _p(me), (C.c_double * 4)(*k), int(job["min_inliers"]), nh, _p(sa), *[_p(a) for a in out])
    return J, (P3, P2, me, sa), out


def pnp_hypotheses(job, device=0):
    """PnPsolver's compute_pose + CheckInliers + Refine for every sample row of one solver (orbx_pnp_hypotheses): job = dict(P3Dw, P2D,
    max_err, K, min_inliers, samples) -> (n_inliers[n_hyp] int32, Rt[n_hyp][12] float64, inlier_bits[n_hyp][(n+63)/64] uint64, n_refined,
    Rt_refined, refined_bits); a row below min_inliers has n_refined = -1"""
    J, keep, out = _pnp_job(job, "pnp_hypotheses")
    _check(lib().orbx_pnp_hypotheses(device, C.byref(J)))
    return out


def pnp_hypotheses_batch(jobs, device=0):
    """orbx_pnp_hypotheses_batch: the solvers of one Relocalization in one upload, one launch, one download -> [as pnp_hypotheses]"""
    nj = len(jobs)
    arr = (PnpJob * max(nj, 1))()
    keep = []
    for j, job in enumerate(jobs):
        J, k, out = _pnp_job(job, "pnp_hypotheses_batch")
        arr[j] = J
        keep.append((J, k, out))
    _check(lib().orbx_pnp_hypotheses_batch(device, arr, nj))
    return [k[2] for k in keep]


def _mono_init_job(job, who, table=True):
    """dict(xy1[n1][2], xy2[n2][2], matches[n][2], K[4] = fx fy cx cy, sigma=1.0, min_parallax=1.0, min_triangulated=50, samples[n_hyp][8])
    -> (MonoInitJob, inputs, table outputs); samples may be absent when table is False"""
    xy1, xy2 = np.ascontiguousarray(job["xy1"], np.float32), np.ascontiguousarray(job["xy2"], np.float32)
    ma = np.ascontiguousarray(job["matches"], np.int32)
    sa = np.ascontiguousarray(job["samples"], np.int32) if job.get("samples") is not None else np.zeros((0, 8), np.int32)
    k = np.asarray(job["K"], np.float32).reshape(-1)
    if xy1.ndim != 2 or xy1.shape[1] != 2 or xy2.ndim != 2 or xy2.shape[1] != 2 or ma.ndim != 2 or ma.shape[1] != 2 or sa.ndim != 2 or \
            sa.shape[1] != 8 or len(k) != 4:
        raise OrbxError(-1, f"{who}: xy1 [n1][2], xy2 [n2][2], matches [n][2], samples [n_hyp][8], K [4]")
    n, nh = len(ma), len(sa)
    words = (n + 63) // 64
    out = (np.zeros(nh, np.float32), np.zeros((nh, 9), np.float32), np.zeros((nh, words), np.uint64),
           np.zeros(nh, np.float32), np.zeros((nh, 9), np.float32), np.zeros((nh, words), np.uint64))
    J = MonoInitJob(len(xy1), len(xy2), _p(xy1), _p(xy2), n, _p(ma), float(job.get("sigma", 1.0)), (C.c_float * 4)(*k),
                    float(job.get("min_parallax", 1.0)), int(job.get("min_triangulated", 50)), nh, _p(sa) if nh else None,
                    _p(out[0]), _p(out[3]), _p(out[1]), _p(out[4]), _p(out[2]), _p(out[5]))
    if not table:
        J.score_h = J.score_f = J.H21 = J.F21 = J.bits_h = J.bits_f = None
    return J, (xy1, xy2, ma, sa), out


def mono_init_hypotheses(job, device=0):
    """The table of Initializer::FindHomography and FindFundamental over the sample rows of one job (orbx_mono_init_hypotheses): job as
    _mono_init_job -> (score_h[n_hyp] float32, H21[n_hyp][9], bits_h[n_hyp][(n+63)/64] uint64, score_f, F21, bits_f)"""
    J, keep, out = _mono_init_job(job, "mono_init_hypotheses")
    _check(lib().orbx_mono_init_hypotheses(device, C.byref(J)))
    return out


def _mono_points(n1):
    return np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8)


def mono_init_reconstruct(job, model, M, mask, device=0):
    """ReconstructH (model 1) / ReconstructF (model 2) on the matrix M[9] and the inlier mask[(n+63)/64] uint64 (orbx_mono_init_reconstruct)
    -> dict(ok, winner, n_good[8], cos_parallax[8], R[8][3][3], t[8][3], P3D[n1][3], triangulated[n1] bool)"""
    J, keep, _ = _mono_init_job(job, "mono_init_reconstruct", table=False)
    M = np.ascontiguousarray(M, np.float32).reshape(-1)
    mask = np.ascontiguousarray(mask, np.uint64).reshape(-1)
    if len(M) != 9 or len(mask) != (J.n + 63) // 64:
        raise OrbxError(-1, "mono_init_reconstruct: M [9], mask [(n+63)/64]")
    P3D, tri = _mono_points(J.n1)
    R = MonoInitRecon(P3D=_p(P3D), triangulated=_p(tri))
    _check(lib().orbx_mono_init_reconstruct(device, C.byref(J), int(model), _p(M), _p(mask), C.byref(R)))
    return dict(ok=bool(R.ok), winner=R.winner, n_good=np.array(R.n_good, np.int32), cos_parallax=np.array(R.cos_parallax, np.float32),
                R=np.array(R.R, np.float32).reshape(8, 3, 3), t=np.array(R.t, np.float32).reshape(8, 3), P3D=P3D, triangulated=tri.astype(bool))


def mono_init_initialize(job, device=0):
    """Initializer::Initialize behind the drawing of the sample rows, in one call (orbx_mono_init_initialize) -> dict(ok, model, best_h,
    best_f, SH, SF, M[9], R21[3][3], t21[3], parallax, winner, n_good[8], cos_parallax[8], P3D[n1][3], triangulated[n1] bool)"""
    J, keep, _ = _mono_init_job(job, "mono_init_initialize", table=False)
    P3D, tri = _mono_points(J.n1)
    R = MonoInitResult(P3D=_p(P3D), triangulated=_p(tri))
    _check(lib().orbx_mono_init_initialize(device, C.byref(J), C.byref(R)))
    return dict(ok=bool(R.ok), model=R.model, best_h=R.best_h, best_f=R.best_f, SH=np.float32(R.SH), SF=np.float32(R.SF),
                M=np.array(R.M, np.float32), R21=np.array(R.R21, np.float32).reshape(3, 3), t21=np.array(R.t21, np.float32),
                parallax=np.float32(R.parallax), winner=R.winner, n_good=np.array(R.n_good, np.int32),
                cos_parallax=np.array(R.cos_parallax, np.float32), P3D=P3D, triangulated=tri.astype(bool))


class DUtilsRandom:
    """DUtils::Random::RandomInt over the C library's rand(), seeded as SeedRandOnce(0) seeds it (Thirdparty/DBoW2/DUtils/Random.cpp):
    the stream Initializer::Initialize draws mvSets from.  seed = None keeps the process's stream (a second SeedRandOnce is a no-op)."""

    def __init__(self, seed=0):
        self._libc = C.CDLL(None)
        if seed is not None:
            self._libc.srand(C.c_uint(seed))

    def random_int(self, lo, hi):
        d = hi - lo + 1
        return int((float(self._libc.rand()) / (2147483647.0 + 1.0)) * d) + lo


def mono_init_draw_sets(n, iterations, rng):
    """mvSets of Initializer::Initialize (:79-111): per iteration eight draws without replacement from 0 .. n-1 -> int32 [iterations][8]"""
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            r = rng.random_int(0, len(avail) - 1)
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


class Initializer:
    """Initializer (reference include/Initializer.h:36-46, src/Initializer.cc:37-145).  keys1 / keys2 = the undistorted keypoint positions
    [n][2] of the reference / current frame, K = mK as 3 x 3 or (fx, fy, cx, cy).  Initialize(keys2, matches12) takes vMatches12 (per
    keypoint of frame 1 the index in frame 2 or -1) and returns (ok, R21[3][3], t21[3], P3D[n1][3], triangulated[n1]); the sample rows are
    drawn as the reference draws them unless `samples` gives them.  self.last keeps the whole result of the call."""

    def __init__(self, keys1, K, sigma=1.0, iterations=200, device=0):
        self.keys1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        K = np.asarray(K, np.float32)
        self.K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32) if K.shape == (3, 3) else K.reshape(4).copy()
        self.sigma, self.iterations, self.device = float(sigma), int(iterations), device
        self.sets = None
        self.last = None

    def Initialize(self, keys2, matches12, samples=None):
        keys2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
        m12 = np.asarray(matches12, np.int64).reshape(-1)
        first = np.nonzero(m12 >= 0)[0]
        matches = np.stack([first, m12[first]], 1).astype(np.int32)
        self.sets = mono_init_draw_sets(len(matches), self.iterations, DUtilsRandom(0)) if samples is None else np.asarray(samples, np.int32)
        r = mono_init_initialize(dict(xy1=self.keys1, xy2=keys2, matches=matches, K=self.K, sigma=self.sigma, samples=self.sets),
                                 self.device)
        self.last = r
        return r["ok"], r["R21"], r["t21"], r["P3D"], r["triangulated"]


class PnPRansac:
    """PnPsolver's RANSAC state machine (reference src/PnPsolver.cc:128-316) over a table of hypotheses.  solver = dict(P3Dw, P2D, sigma2,
    K, samples): mvP3Dw, mvP2D, mvSigma2, (fu, fv, uc, vc) and the sample rows, four distinct indices each, drawn by the caller (the
    swap-remove draw of :199-212 from a generator of the caller's: a stated deviation from DUtils::Random).  indices = mvKeyPointIndices and
    n_matches = mvpMapPointMatches.size() scatter the inliers as the reference does.  The first iterate() or find() evaluates the first
    mRansacMaxIts rows on the device in one call -- the reference's loop condition is an OR, so the first call walks them all unless a
    refinement returns early -- and rows beyond them in blocks of n, by a second small call, only when the replay reaches them.
    pnp_hypotheses_batch([r.table_job() for r in solvers]) + r.set_table(...) evaluates several solvers in one launch."""

    def __init__(self, solver, indices=None, n_matches=None, device=0):
        self.solver, self.device = solver, device
        self.N = len(solver["P3Dw"])
        self.indices = np.arange(self.N) if indices is None else np.asarray(indices, np.int64)
        self.n_matches = self.N if n_matches is None else int(n_matches)
        self.iterations = 0
        self.best_inliers, self.best, self.best_row = 0, None, -1
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991):
        import math
        N, f32 = self.N, np.float32
        eps = f32(epsilon)
        n_min = max(int(f32(N) * eps), min_inliers, min_set)          # int nMinInliers = N*mRansacEpsilon: a float product, truncated
        with np.errstate(all="ignore"):
            if eps < f32(n_min) / f32(N):
                eps = f32(n_min) / f32(N)
            n_it = 1
            if n_min != N:
                x = np.log(np.float64(1.0) - np.float64(probability)) / np.log(np.float64(1.0) - np.float64(math.pow(float(eps), 3.0)))
                n_it = int(math.ceil(float(x))) if np.isfinite(x) else -2 ** 31
        self.min_inliers, self.epsilon = n_min, eps
        self.max_its = max(1, min(n_it, max_iterations))
        self.max_err = (np.asarray(self.solver["sigma2"], f32) * f32(th2)).astype(f32)
        self.table = None

    def table_job(self, lo=0, hi=None):
        """the job of rows lo .. hi-1 (default: the first mRansacMaxIts)"""
        hi = self.max_its if hi is None else hi
        sa = np.asarray(self.solver["samples"])
        if len(sa) < hi:
            raise OrbxError(-1, f"PnPRansac: {len(sa)} sample rows, row {hi - 1} is needed")
        return dict(P3Dw=self.solver["P3Dw"], P2D=self.solver["P2D"], max_err=self.max_err, K=self.solver["K"], min_inliers=self.min_inliers,
                    samples=sa[lo:hi])

    def set_table(self, table):
        self.table = tuple(np.asarray(a) for a in table)

    def _bits(self, words):
        return np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8), bitorder="little")[:self.N].astype(bool)

    def _need(self, k, block):
        if self.table is None:
            self.set_table(pnp_hypotheses(self.table_job(), self.device))
        have = len(self.table[0])
        if k >= have:      # the lazy tail: a solver called again past mRansacMaxIts
            more = pnp_hypotheses(self.table_job(have, max(k + 1, have + block)), self.device)
            self.table = tuple(np.concatenate([a, b]) for a, b in zip(self.table, more))

    def _scatter(self, inl):
        vb = np.zeros(self.n_matches, bool)
        vb[self.indices[inl]] = True
        return vb

    @staticmethod
    def Tcw(rt):
        """mBestTcw / mRefinedTcw: the CV_64F -> CV_32F conversion of :228-234"""
        T = np.eye(4, dtype=np.float32)
        with np.errstate(all="ignore"):
            T[:3, :3] = rt[:9].astype(np.float32).reshape(3, 3)
            T[:3, 3] = rt[9:12].astype(np.float32)
        return T

    def iterate(self, n_iterations):
        """-> (Tcw 4 x 4 float32 or None, bNoMore, vbInliers[n_matches], nInliers)"""
        vb = np.zeros(self.n_matches, bool)
        if self.N < self.min_inliers:
            return None, True, vb, 0
        cur = 0
        while self.iterations < self.max_its or cur < n_iterations:
            cur += 1
            self.iterations += 1
            k = self.iterations - 1
            self._need(k, max(1, n_iterations))
            ni, rt, bits, nr, rtr, rbits = self.table
            if ni[k] >= self.min_inliers:
                if ni[k] > self.best_inliers:
                    self.best_inliers, self.best, self.best_row = int(ni[k]), (rt[k].copy(), self._bits(bits[k])), k
                # Refine reads mvbBestInliers: the best row's own refinement, already in the table
                b = self.best_row
                if nr[b] > self.min_inliers:
                    return self.Tcw(rtr[b]), False, self._scatter(self._bits(rbits[b])), int(nr[b])
        if self.iterations >= self.max_its:
            if self.best_inliers >= self.min_inliers:
                return self.Tcw(self.best[0]), True, self._scatter(self.best[1]), self.best_inliers
            return None, True, vb, 0
        return None, False, vb, 0

    def find(self):
        T, _, vb, ni = self.iterate(self.max_its)
        return T, vb, ni


def _pose_cam(pose, cam, who):
    po = np.ascontiguousarray(pose, np.float32).reshape(-1); ca = np.ascontiguousarray(cam, np.float32).reshape(-1)
    if len(po) != 15 or len(ca) != 9:
        raise OrbxError(-1, f"{who}: pose is Rcw[9] tcw[3] Ow[3], cam is fx fy cx cy mbf mnMinX mnMinY mnMaxX mnMaxY")
    return po, ca


def _occupied_for(occupied, frame, who):
    """per-call occupied bytes of a resident frame (None: no feature occupied); one byte per feature of THAT frame"""
    if occupied is None:
        return None
    oc = np.ascontiguousarray(occupied, np.uint8)
    if oc.ndim != 1 or len(oc) != frame.n:
        raise OrbxError(-1, f"{who}: occupied has {oc.size} entries, the frame has {frame.n} features")
    return oc


class BowDatabase:
    """Device-resident keyframe set (include/orbx.h: orbx_bowdb_*): upload once, search many frames."""

    def __init__(self, keyframes, device=0):
        self._L = lib()
        sets = [make_featset(k) for k in keyframes]
        arr = (FeatSet * len(sets))(*[s_[0] for s_ in sets])
        self._h = C.c_void_p()
        _check(self._L.orbx_bowdb_create(device, arr, len(sets), C.byref(self._h)))
        self.nkf = len(sets)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.orbx_bowdb_destroy(h)
            self._h = None

    def search(self, F, nnratio=0.75, checkOri=True):
        b, kb = make_featset(F)
        nkf = self._L.orbx_bowdb_size(self._h)
        out = np.full((nkf, b.n), -1, np.int32); n = np.zeros(nkf, np.int32)
        _check(self._L.orbx_bowdb_search(self._h, C.byref(b), nnratio, int(checkOri), _p(out), _p(n)))
        return out, n

    # ---- the live set (orbx_bowdb_create_live): keyframes enter, leave and change flags while it is searched
    @classmethod
    def live(cls, max_kf, cap, max_ids, device=0):
        """an empty set of max_kf slots of `cap` features for ids in [0, max_ids); BowFrames.search* take it as they take an immutable one
        (the candidate searches with kf_of_id=None: the set keeps the id map itself)"""
        self = cls.__new__(cls)
        self._L = lib()
        self._h = C.c_void_p()
        _check(self._L.orbx_bowdb_create_live(device, int(max_kf), int(cap), int(max_ids), C.byref(self._h)))
        self.max_kf, self.cap, self.max_ids, self.device = int(max_kf), int(cap), int(max_ids), device
        return self

    def size(self):
        """keyframes (an immutable set) or slots ever used (a live one): the rows the all-keyframes searches write (orbx_bowdb_size)"""
        return self._L.orbx_bowdb_size(self._h)

    def add_from_frames(self, id, frames, index, d_flag=None, stream=None):
        """keyframe `id` from slot `index` of a BowFrames, device to device and asynchronous; d_flag = device uint8[cap] or None (all set)"""
        _check(self._L.orbx_bowdb_add_from_frames(self._h, int(id), frames._h, int(index), d_flag, stream))

    def add(self, id, keyframe, stream=None):
        """keyframe `id` from a host feature set (the dict BowDatabase(...) takes)"""
        b, kb = make_featset(keyframe)
        _check(self._L.orbx_bowdb_add(self._h, int(id), C.byref(b), stream))

    def erase(self, id, stream=None):
        _check(self._L.orbx_bowdb_erase(self._h, int(id), stream))

    def set_flags(self, ids, flags, stream=None):
        """new map-point flags (uint8 per feature) for the live keyframes `ids`, one launch.  The mirror first asks the set for each
        keyframe's feature count (a small synchronising read per keyframe) to refuse an array of another length; a caller that cannot
        afford that calls orbx_bowdb_set_flags itself, as tools/bench_live_bowdb.py does"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        if len(flags) != len(ids):
            raise OrbxError(-1, f"set_flags: {len(ids)} ids, {len(flags)} flag arrays")
        keep = [np.ascontiguousarray(f, np.uint8).reshape(-1) for f in flags]
        for k, a in zip(ids, keep):           # the C entry reads as many bytes as the keyframe has features
            n = C.c_int(-1)
            _check(self._L.orbx_bowdb_read_keyframe(self._h, int(k), C.byref(n), None, None, None, None, None, None, None, None, None))
            if len(a) != n.value:
                raise OrbxError(-1, f"set_flags: {len(a)} flags for keyframe {int(k)} of {n.value} features")
        ptrs = (C.c_void_p * max(len(keep), 1))(*[a.ctypes.data for a in keep])
        _check(self._L.orbx_bowdb_set_flags(self._h, _p(ids), len(ids), ptrs, stream))

    def live_count(self):
        rc = self._L.orbx_bowdb_live_count(self._h)
        if rc < 0:
            _check(rc)
        return rc

    def ids(self):
        """the id behind every slot, -1 = empty (int32[size()])"""
        out = np.full(self.size(), -1, np.int32)
        _check(self._L.orbx_bowdb_ids(self._h, _p(out), len(out)))
        return out

    def read_keyframe(self, id):
        """the searched form of keyframe `id` as the kernels see it: dict(n, nnodes, node_id, node_off, feat, flag, angle, desc, sdesc, sflag),
        the filtered arrays cut to the filtered length"""
        cap = self.cap
        n, nn = C.c_int(), C.c_int()
        node_id = np.zeros(cap, np.uint32); node_off = np.zeros(cap + 1, np.int32); feat = np.zeros(cap, np.uint32)
        flag = np.zeros(cap, np.uint8); angle = np.zeros(cap, np.float32); desc = np.zeros((cap, 32), np.uint8)
        sdesc = np.zeros((cap, 32), np.uint8); sflag = np.zeros(cap, np.uint8)
        _check(self._L.orbx_bowdb_read_keyframe(self._h, int(id), C.byref(n), C.byref(nn), _p(node_id), _p(node_off), _p(feat), _p(flag),
                                                _p(angle), _p(desc), _p(sdesc), _p(sflag)))
        n, nn = n.value, nn.value
        m = int(node_off[nn])
        return dict(n=n, nnodes=nn, node_id=node_id[:nn].copy(), node_off=node_off[:nn + 1].copy(), feat=feat[:m].copy(), flag=flag[:n].copy(),
                    angle=angle[:n].copy(), desc=desc[:n].copy(), sdesc=sdesc[:m].copy(), sflag=sflag[:m].copy())


class BowFrames:
    """Device-resident Frame::ComputeBoW results of a batch of frames (include/orbx.h: orbx_bow_frames_*)."""

    def __init__(self, max_batch, cap, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        _check(self._L.orbx_bow_frames_create(device, max_batch, cap, C.byref(self._h)))
        self.batch, self.cap = max_batch, cap

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.orbx_bow_frames_destroy(h)
            self._h = None

    def transform(self, voc, d_kps, d_desc, d_n, batch, levelsup=4, stream=None):
        """device pointers of orbx_extract_batch_device's outputs -> BowVector / FeatureVector in HBM (asynchronous)"""
        _check(self._L.orbx_bow_transform_batch_device(voc._h, self._h, d_kps, d_desc, d_n, batch, levelsup, stream))

    def read(self, index, stream=None):
        cap = self.cap
        bid = np.zeros(cap, np.uint32); bval = np.zeros(cap, np.float64); nb = C.c_int()
        fid = np.zeros(cap, np.uint32); foff = np.zeros(cap + 1, np.int32); ffeat = np.zeros(cap, np.uint32); fn = C.c_int()
        _check(self._L.orbx_bow_frames_read(self._h, index, stream, _p(bid), _p(bval), C.byref(nb), _p(fid), _p(foff), _p(ffeat), C.byref(fn)))
        return dict(bow_id=bid[:nb.value].copy(), bow_val=bval[:nb.value].copy(), fv_node_id=fid[:fn.value].copy(),
                    fv_node_off=foff[:fn.value + 1].copy(), fv_feat=ffeat[:foff[fn.value]].copy())

    def set_bow(self, index, bow, stream=None):
        """a host BowVector into slot `index` (orbx_bow_frames_set_bow); the slot's FeatureVector is left alone"""
        bid, bval = _bow_query(bow)
        _check(self._L.orbx_bow_frames_set_bow(self._h, int(index), _p(bid), _p(bval), len(bid), stream))

    def search(self, db, batch, d_match, d_nmatches, nnratio=0.75, checkOri=True, stream=None):
        """every keyframe of a BowDatabase against frames 0..batch-1: d_match[batch][nkf][cap], d_nmatches[batch][nkf] (device)"""
        _check(self._L.orbx_bowdb_search_batch_device(db._h, self._h, batch, nnratio, int(checkOri), d_match, d_nmatches, stream))

    def search_compact(self, db, batch, d_pairs, cap_pairs, d_nmatches, nnratio=0.75, checkOri=True, stream=None):
        """the same search with compact results: d_pairs[batch][nkf][cap_pairs][2] int32 = (frame feature, keyframe feature) in frame-feature order,
        d_nmatches[batch][nkf] = counts (orbx_bowdb_search_batch_device_compact)"""
        _check(self._L.orbx_bowdb_search_batch_device_compact(db._h, self._h, batch, nnratio, int(checkOri), d_pairs, int(cap_pairs), d_nmatches, stream))

    def search_candidates(self, db, batch, d_cand, cand_stride, d_ncand, d_match, d_nmatches, nnratio=0.75, checkOri=True, kf_of_id=None, n_ids=0,
                          stream=None):
        """frames 0..batch-1 against the keyframes their candidate lists name -- d_cand[batch][cand_stride], d_ncand[batch], device int32 as
        KeyFrameDatabase.detect_relocalization_batch_device leaves them -- in one launch, the lists read on the device:
        d_match[batch][cand_stride][cap], d_nmatches[batch][cand_stride] (-1 = slot not searched).  kf_of_id: optional device int32[n_ids], id ->
        index into db (-1 = not in it); None: an id is the index (orbx_bowdb_search_candidates_device)"""
        _check(self._L.orbx_bowdb_search_candidates_device(db._h, self._h, int(batch), d_cand, int(cand_stride), d_ncand, kf_of_id, int(n_ids), nnratio,
                                                           int(checkOri), d_match, d_nmatches, stream))

    def search_candidates_compact(self, db, batch, d_cand, cand_stride, d_ncand, d_pairs, cap_pairs, d_nmatches, nnratio=0.75, checkOri=True,
                                  kf_of_id=None, n_ids=0, stream=None):
        """the same with compact results: d_pairs[batch][cand_stride][cap_pairs][2] as search_compact writes them per keyframe
        (orbx_bowdb_search_candidates_device_compact)"""
        _check(self._L.orbx_bowdb_search_candidates_device_compact(db._h, self._h, int(batch), d_cand, int(cand_stride), d_ncand, kf_of_id, int(n_ids),
                                                                   nnratio, int(checkOri), d_pairs, int(cap_pairs), d_nmatches, stream))


def _bow_query(bow):
    """(bow_id, bow_val) or dict(bow_id=, bow_val=) -> contiguous (uint32 ids, float64 values)"""
    if isinstance(bow, dict):
        bow = (bow["bow_id"], bow["bow_val"])
    bid = np.ascontiguousarray(bow[0], np.uint32).reshape(-1); bval = np.ascontiguousarray(bow[1], np.float64).reshape(-1)
    if len(bid) != len(bval):
        raise OrbxError(-1, f"BowVector: {len(bid)} word ids, {len(bval)} values")
    return bid, bval


class KeyFrameDatabase:
    """Mirror of ORB_SLAM2::KeyFrameDatabase (reference include/KeyFrameDatabase.h:42-70) over orbx_kfdb_*: the keyframes' BowVectors,
    covisibility neighbours and relocalisation scores live in HBM.  Keyframes are named by the id `add` returns (the add sequence number).
    A query is a host BowVector -- (bow_id, bow_val) or a dict with those keys -- or (BowFrames, index)."""

    def __init__(self, nwords, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        _check(self._L.orbx_kfdb_create(device, int(nwords), C.byref(self._h)))
        self.device = device

    def __del__(self):
        try:
            h, L = getattr(self, "_h", None), _lib
            if h and L is not None:
                L.orbx_kfdb_destroy(h)
            self._h = None
        except Exception:
            pass

    def __len__(self):
        return self._L.orbx_kfdb_size(self._h)

    def next_id(self):
        return self._L.orbx_kfdb_next_id(self._h)

    def clear(self):
        _check(self._L.orbx_kfdb_clear(self._h))

    def add(self, bow, index=None, stream=None):
        """add(host BowVector) or add(BowFrames, index): -> id"""
        out = C.c_int(-1)
        if isinstance(bow, BowFrames):
            _check(self._L.orbx_kfdb_add_from_frames(self._h, bow._h, int(index), stream, C.byref(out)))
        else:
            bid, bval = _bow_query(bow)
            _check(self._L.orbx_kfdb_add(self._h, _p(bid), _p(bval), len(bid), C.byref(out)))
        return out.value

    def erase(self, id):
        _check(self._L.orbx_kfdb_erase(self._h, int(id)))

    def set_covisibility(self, id, neighbours):
        nb = np.ascontiguousarray(neighbours, np.int32).reshape(-1)
        _check(self._L.orbx_kfdb_set_covisibility(self._h, int(id), _p(nb), len(nb)))

    def reloc_scores(self):
        out = np.zeros(self.next_id(), np.float32)
        _check(self._L.orbx_kfdb_reloc_scores(self._h, _p(out), len(out)))
        return out

    def score(self, query, ids, index=None):
        """ORBVocabulary::score(query, keyframe) for every id: float64, bit-exact"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        out = np.zeros(len(ids), np.float64)
        if isinstance(query, BowFrames):
            _check(self._L.orbx_kfdb_score_frame(self._h, query._h, int(index), _p(ids), len(ids), _p(out)))
        else:
            bid, bval = _bow_query(query)
            _check(self._L.orbx_kfdb_score(self._h, _p(bid), _p(bval), len(bid), _p(ids), len(ids), _p(out)))
        return out

    def _detect(self, query, index, loop, connected, min_score, cap, stages):
        n = self.next_id()
        cap = n if cap is None else int(cap)
        cand = np.zeros(max(cap, 1), np.int32); nc = C.c_int(0)
        words = np.zeros(n, np.int32) if stages else None
        score = np.zeros(n, np.float32) if stages else None
        conn = np.ascontiguousarray(connected if connected is not None else [], np.int32).reshape(-1)
        L = self._L
        if isinstance(query, BowFrames):
            if loop:
                rc = L.orbx_kfdb_detect_loop_frame(self._h, query._h, int(index), _p(conn), len(conn), float(min_score), _p(cand), cap, C.byref(nc), _p(words), _p(score))
            else:
                rc = L.orbx_kfdb_detect_relocalization_frame(self._h, query._h, int(index), _p(cand), cap, C.byref(nc), _p(words), _p(score))
        else:
            bid, bval = _bow_query(query)
            if loop:
                rc = L.orbx_kfdb_detect_loop(self._h, _p(bid), _p(bval), len(bid), _p(conn), len(conn), float(min_score), _p(cand), cap, C.byref(nc), _p(words), _p(score))
            else:
                rc = L.orbx_kfdb_detect_relocalization(self._h, _p(bid), _p(bval), len(bid), _p(cand), cap, C.byref(nc), _p(words), _p(score))
        if rc != 0:
            e = OrbxError(rc, L.orbx_last_error().decode(errors="replace"))
            e.ncand = nc.value               # ORBX_E_CAPACITY: the true count
            raise e
        out = [int(v) for v in cand[:nc.value]]
        return (out, words, score) if stages else out

    def DetectRelocalizationCandidates(self, F, index=None, cap=None, stages=False):
        """-> candidate ids in the reference's order (stages=True: also words[id], score[id] of this query)"""
        return self._detect(F, index, False, None, 0.0, cap, stages)

    def DetectLoopCandidates(self, pKF, connected, minScore, index=None, cap=None, stages=False):
        """pKF: the query keyframe's BowVector; connected: ids of pKF->GetConnectedKeyFrames()"""
        return self._detect(pKF, index, True, connected, minScore, cap, stages)

    def detect_relocalization_batch_device(self, frames, batch, d_cand, cap, d_ncand, stream=None):
        """frames 0..batch-1 of a BowFrames as relocalisation queries, results in device memory: d_cand[batch][cap] int32, d_ncand[batch]
        int32 (true counts); asynchronous on `stream`"""
        _check(self._L.orbx_kfdb_detect_relocalization_batch_device(self._h, frames._h, int(batch), d_cand, int(cap), d_ncand, stream))


class ORBmatcher:
    """Mirror of ORB_SLAM2::ORBmatcher (reference include/ORBmatcher.h:41-103) for the searches on the
    north-star path.  Feature sets are dicts as accepted by make_featset()."""
    TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30  # src/ORBmatcher.cc:37-39

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.mfNNratio, self.mbCheckOrientation, self.device = float(nnratio), bool(checkOri), device

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
        return lib().orbx_hamming(_p(a), _p(b))

    def SearchByBoW(self, pKF, other, frame=None):
        """SearchByBoW(pKF, F) when `other` is a frame feature set (kind='frame', default) ->
        (match_f, nmatches); SearchByBoW(pKF1, pKF2) when other['kind']=='keyframe' -> (match12, nmatches)."""
        a, ka = make_featset(pKF); b, kb = make_featset(other)
        n = C.c_int()
        if other.get("kind", "frame") == "keyframe":
            out = np.full(a.n, -1, np.int32)
            _check(lib().orbx_search_by_bow_kf_kf(self.device, C.byref(a), C.byref(b), self.mfNNratio, int(self.mbCheckOrientation), _p(out), C.byref(n)))
        else:
            out = np.full(b.n, -1, np.int32)
            _check(lib().orbx_search_by_bow_kf_f(self.device, C.byref(a), C.byref(b), self.mfNNratio, int(self.mbCheckOrientation), _p(out), C.byref(n)))
        return out, n.value

    def SearchByBoWBatch(self, keyframes, F):
        """Relocalization loop (src/Tracking.cc:1661-1682): every keyframe against one frame."""
        sets = [make_featset(k) for k in keyframes]
        arr = (FeatSet * len(sets))(*[s[0] for s in sets])
        b, kb = make_featset(F)
        out = np.full((len(sets), b.n), -1, np.int32); n = np.zeros(len(sets), np.int32)
        _check(lib().orbx_search_by_bow_kf_f_batch(self.device, arr, len(sets), C.byref(b), self.mfNNratio, int(self.mbCheckOrientation), _p(out), _p(n)))
        return out, n

    def SearchByBoWKeyFrames(self, pKF1, keyframes2):
        """LoopClosing::ComputeSim3's loop (src/LoopClosing.cc:293-323): SearchByBoW(pKF1, pKF2) for every candidate in
        one call -> (match12[n2, n1], nmatches[n2])"""
        a, ka = make_featset(pKF1)
        sets = [make_featset(k) for k in keyframes2]
        arr = (FeatSet * len(sets))(*[s[0] for s in sets])
        out = np.full((len(sets), a.n), -1, np.int32); n = np.zeros(len(sets), np.int32)
        _check(lib().orbx_search_by_bow_kf_kf_batch(self.device, C.byref(a), arr, len(sets), self.mfNNratio, int(self.mbCheckOrientation), _p(out), _p(n)))
        return out, n

    def SearchForTriangulationBatch(self, pKF1, keyframes2, F12s, epipoles, scaleFactors2, levelSigma2_2, bOnlyStereo=False):
        """LocalMapping::CreateNewMapPoints' loop (src/LocalMapping.cc:241-309): the current keyframe against every neighbour in
        one call -> list of (npairs_i, 2) arrays"""
        a, ka = make_featset(pKF1)
        sets = [make_featset(k) for k in keyframes2]
        arr = (FeatSet * len(sets))(*[s[0] for s in sets])
        F = np.ascontiguousarray(np.asarray(F12s, np.float32).reshape(len(sets), 9))
        ep = np.ascontiguousarray(np.asarray(epipoles, np.float32).reshape(len(sets), 2))
        sf = np.ascontiguousarray(scaleFactors2, np.float32); sg = np.ascontiguousarray(levelSigma2_2, np.float32)
        cap = max(a.n, 1)
        pairs = np.zeros((len(sets), cap, 2), np.int32); n = np.zeros(len(sets), np.int32)
        _check(lib().orbx_search_for_triangulation_batch(self.device, C.byref(a), arr, len(sets), _p(F), _p(ep), _p(sf), _p(sg), len(sf),
                                                         int(bOnlyStereo), int(self.mbCheckOrientation), _p(pairs), cap, _p(n)))
        return [pairs[i, :n[i]].copy() for i in range(len(sets))]

    # ---- the same searches on resident keyframes (DeviceKeyFrame): flags travel per call
    def SearchByBoWResident(self, kf, kf_flag, frame):
        """SearchByBoW(pKF, F) with both sides resident -> (match_f, nmatches)"""
        fl = _flags_for(kf_flag, kf, "SearchByBoWResident")
        out = np.full(frame.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_kf_search_by_bow_kf_f(kf._h, _p(fl), frame._h, self.mfNNratio, int(self.mbCheckOrientation), _p(out), C.byref(n)))
        return out, n.value

    def SearchByBoWKeyFramesFrameResident(self, kfs, kf_flags, frame):
        """Tracking::Relocalization's loop (src/Tracking.cc:1661-1682) as one call: SearchByBoW(pKF, F) for every resident keyframe of `kfs`
        against one frame given as a host feature set (dict) -> (match_f[nkf][nF], nmatches[nkf])"""
        if len(kf_flags) != len(kfs):
            raise OrbxError(-1, "SearchByBoWKeyFramesFrameResident: one flag array per keyframe")
        fl = [_flags_for(x, k, "SearchByBoWKeyFramesFrameResident") for x, k in zip(kf_flags, kfs)]
        hs = (C.c_void_p * len(kfs))(*[k._h for k in kfs])
        fp = (C.c_void_p * len(kfs))(*[x.ctypes.data for x in fl])
        fs, keep = make_featset(frame)
        out = np.full((len(kfs), fs.n), -1, np.int32); n = np.zeros(len(kfs), np.int32)
        _check(lib().orbx_kf_search_by_bow_kfs_f(hs, fp, len(kfs), C.byref(fs), self.mfNNratio, int(self.mbCheckOrientation), _p(out), _p(n)))
        return out, n

    def SearchByBoWKeyFramesResident(self, kf1, flag1, kfs2, flags2):
        f1 = _flags_for(flag1, kf1, "SearchByBoWKeyFramesResident")
        if len(flags2) != len(kfs2):
            raise OrbxError(-1, "SearchByBoWKeyFramesResident: one flag array per second keyframe")
        f2 = [_flags_for(x, k, "SearchByBoWKeyFramesResident") for x, k in zip(flags2, kfs2)]
        hs = (C.c_void_p * len(kfs2))(*[k._h for k in kfs2])
        fp = (C.c_void_p * len(kfs2))(*[x.ctypes.data for x in f2])
        out = np.full((len(kfs2), kf1.n), -1, np.int32); n = np.zeros(len(kfs2), np.int32)
        _check(lib().orbx_kf_search_by_bow_kf_kf(kf1._h, _p(f1), hs, fp, len(kfs2), self.mfNNratio, int(self.mbCheckOrientation), _p(out), _p(n)))
        return out, n

    def SearchForTriangulationResident(self, kf1, flag1, kfs2, flags2, F12s, epipoles, scaleFactors2, levelSigma2_2, bOnlyStereo=False):
        f1 = _flags_for(flag1, kf1, "SearchForTriangulationResident") if flag1 is not None else None
        if flags2 is not None and len(flags2) != len(kfs2):
            raise OrbxError(-1, "SearchForTriangulationResident: one flag array per second keyframe")
        f2 = [_flags_for(x, k, "SearchForTriangulationResident") for x, k in zip(flags2, kfs2)] if flags2 is not None else None
        hs = (C.c_void_p * len(kfs2))(*[k._h for k in kfs2])
        fp = (C.c_void_p * len(kfs2))(*[x.ctypes.data for x in f2]) if f2 is not None else None
        F = np.ascontiguousarray(np.asarray(F12s, np.float32).reshape(len(kfs2), 9))
        ep = np.ascontiguousarray(np.asarray(epipoles, np.float32).reshape(len(kfs2), 2))
        sf = np.ascontiguousarray(scaleFactors2, np.float32); sg = np.ascontiguousarray(levelSigma2_2, np.float32)
        cap = max(kf1.n, 1)
        pairs = np.zeros((len(kfs2), cap, 2), np.int32); n = np.zeros(len(kfs2), np.int32)
        _check(lib().orbx_kf_search_for_triangulation(kf1._h, _p(f1), hs, fp, len(kfs2), _p(F), _p(ep), _p(sf), _p(sg), len(sf),
                                                      int(bOnlyStereo), int(self.mbCheckOrientation), _p(pairs), cap, _p(n)))
        return [pairs[i, :n[i]].copy() for i in range(len(kfs2))]

    @staticmethod
    def _frame(d):
        keep = {}
        def arr(k, dt):
            keep[k] = np.ascontiguousarray(d[k], dtype=dt); return keep[k].ctypes.data
        s_ = FrameFeats()
        s_.x = arr("x", np.float32); s_.y = arr("y", np.float32); s_.octave = arr("octave", np.int32); s_.angle = arr("angle", np.float32)
        s_.u_right = arr("u_right", np.float32); s_.desc = arr("desc", np.uint8)
        s_.occupied = arr("occupied", np.uint8) if d.get("occupied") is not None else None
        s_.n = len(keep["x"])
        s_.min_x, s_.min_y, s_.max_x, s_.max_y = [float(v) for v in d["bounds"]]
        return s_, keep

    @staticmethod
    def _points(d):
        keep = {}
        def arr(k, dt):
            if d.get(k) is None:
                return None
            keep[k] = np.ascontiguousarray(d[k], dtype=dt); return keep[k].ctypes.data
        s_ = ProjPoints()
        s_.u = arr("u", np.float32); s_.v = arr("v", np.float32); s_.aux = arr("aux", np.float32); s_.level = arr("level", np.int32)
        s_.angle = arr("angle", np.float32); s_.view_cos = arr("view_cos", np.float32); s_.desc = arr("desc", np.uint8)
        s_.valid = arr("valid", np.uint8); s_.has_obs = arr("has_obs", np.uint8)
        s_.n = len(keep["u"])
        return s_, keep

    def SearchByProjectionLastFrame(self, CurrentFrame, LastFramePoints, scaleFactors, th, direction=0, mbf=0.0):
        """SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono), src/ORBmatcher.cc:1396-1553
        -> (match_cur, nmatches)"""
        a, ka = self._frame(CurrentFrame); b, kb = self._points(LastFramePoints)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        out = np.full(a.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_search_by_projection_last_frame(self.device, C.byref(a), C.byref(b), _p(sf), len(sf), th, direction, mbf,
                                                          int(self.mbCheckOrientation), _p(out), C.byref(n)))
        return out, n.value

    def SearchByProjectionMapPoints(self, F, vpMapPoints, scaleFactors, th=3.0):
        """SearchByProjection(Frame &F, const vector<MapPoint*>&, th), src/ORBmatcher.cc:48-129 -> (match_cur, nmatches)"""
        a, ka = self._frame(F); b, kb = self._points(vpMapPoints)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        out = np.full(a.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_search_by_projection_map_points(self.device, C.byref(a), C.byref(b), _p(sf), len(sf), th, self.mfNNratio,
                                                          _p(out), C.byref(n)))
        return out, n.value

    def SearchByProjectionKeyFrame(self, CurrentFrame, KFPoints, scaleFactors, th, ORBdist):
        """SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist), src/ORBmatcher.cc:1555-1685
        -> (match_cur, nmatches)"""
        a, ka = self._frame(CurrentFrame); b, kb = self._points(KFPoints)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        out = np.full(a.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_search_by_projection_keyframe(self.device, C.byref(a), C.byref(b), _p(sf), len(sf), th, int(ORBdist),
                                                        int(self.mbCheckOrientation), _p(out), C.byref(n)))
        return out, n.value

    # ---- the per-frame searches on a resident frame (DeviceFrame): only the points and `occupied` travel per call
    def SearchByProjectionLastFrameResident(self, frame, occupied, LastFramePoints, scaleFactors, th, direction=0, mbf=0.0, check_orientation=None):
        """SearchByProjectionLastFrame on a DeviceFrame; check_orientation (0, 1, 3) defaults to mbCheckOrientation -> (match_cur, nmatches)"""
        oc = _occupied_for(occupied, frame, "SearchByProjectionLastFrameResident")
        b, kb = self._points(LastFramePoints)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        co = int(self.mbCheckOrientation) if check_orientation is None else int(check_orientation)
        out = np.full(frame.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_frame_search_by_projection_last_frame(frame._h, None if oc is None else _p(oc), C.byref(b), _p(sf), len(sf), th,
                                                                direction, mbf, co, _p(out), C.byref(n)))
        return out, n.value

    def SearchByProjectionMapPointsResident(self, frame, occupied, vpMapPoints, scaleFactors, th=3.0):
        oc = _occupied_for(occupied, frame, "SearchByProjectionMapPointsResident")
        b, kb = self._points(vpMapPoints)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        out = np.full(frame.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_frame_search_by_projection_map_points(frame._h, None if oc is None else _p(oc), C.byref(b), _p(sf), len(sf), th,
                                                                self.mfNNratio, _p(out), C.byref(n)))
        return out, n.value

    def SearchByProjectionKeyFrameResident(self, frame, occupied, KFPoints, scaleFactors, th, ORBdist, check_orientation=None):
        oc = _occupied_for(occupied, frame, "SearchByProjectionKeyFrameResident")
        b, kb = self._points(KFPoints)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        co = int(self.mbCheckOrientation) if check_orientation is None else int(check_orientation)
        out = np.full(frame.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_frame_search_by_projection_keyframe(frame._h, None if oc is None else _p(oc), C.byref(b), _p(sf), len(sf), th,
                                                              int(ORBdist), co, _p(out), C.byref(n)))
        return out, n.value

    def SearchByProjectionSim3(self, pKF, vpPoints, scaleFactors, th):
        """SearchByProjection(KeyFrame *pKF, Scw, vpPoints, vpMatched, th), src/ORBmatcher.cc:305-415 -> (match_kf, nmatches)"""
        a, ka = self._frame(pKF); b, kb = self._points(vpPoints)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        out = np.full(a.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_search_by_projection_sim3(self.device, C.byref(a), C.byref(b), _p(sf), len(sf), th, _p(out), C.byref(n)))
        return out, n.value

    def Fuse(self, pKF, vpMapPoints, scaleFactors, invLevelSigma2=None, th=3.0, max_dist=50):
        """search half of both Fuse overloads (src/ORBmatcher.cc:873-1164): invLevelSigma2 given -> the chi2-gated
        variant of Fuse(pKF, vpMapPoints, th).  -> (best_idx, best_dist, nfound)"""
        a, ka = self._frame(pKF); b, kb = self._points(vpMapPoints)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        sg = None if invLevelSigma2 is None else np.ascontiguousarray(invLevelSigma2, np.float32)
        bi = np.full(b.n, -1, np.int32); bd = np.full(b.n, 256, np.int32); n = C.c_int()
        _check(lib().orbx_window_best(self.device, C.byref(a), C.byref(b), _p(sf), None if sg is None else _p(sg), len(sf), th,
                                      0 if sg is None else 1, int(max_dist), _p(bi), _p(bd), C.byref(n)))
        return bi, bd, n.value

    # ---- the keyframe searches on resident keyframes (DeviceFrame as the keyframe): only the points travel per call; safe from several
    # threads on one DeviceFrame (ctypes releases the GIL during the call)
    def FuseResident(self, kf, vpMapPoints, scaleFactors, invLevelSigma2=None, th=3.0, max_dist=50):
        """Fuse's search half on a DeviceFrame (orbx_frame_window_best) -> (best_idx, best_dist, nfound)"""
        b, kb = self._points(vpMapPoints)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        sg = None if invLevelSigma2 is None else np.ascontiguousarray(invLevelSigma2, np.float32)
        bi = np.full(b.n, -1, np.int32); bd = np.full(b.n, 256, np.int32); n = C.c_int()
        _check(lib().orbx_frame_window_best(kf._h, C.byref(b), _p(sf), None if sg is None else _p(sg), len(sf), th, 0 if sg is None else 1,
                                            int(max_dist), _p(bi), _p(bd), C.byref(n)))
        return bi, bd, n.value

    def FuseResidentBatch(self, jobs):
        """jobs: dicts with kf (DeviceFrame), points, scaleFactors and optionally invLevelSigma2 (given: the chi2-gated variant), th (3.0),
        max_dist (50) -- one upload, one launch, one download (orbx_frame_window_best_batch) -> [(best_idx, best_dist, nfound), ...]"""
        arr = (WindowJob * max(len(jobs), 1))()
        keep, outs = [], []
        for j, jb in enumerate(jobs):
            b, kb = self._points(jb["points"])
            sf = np.ascontiguousarray(jb["scaleFactors"], np.float32)
            sg = None if jb.get("invLevelSigma2") is None else np.ascontiguousarray(jb["invLevelSigma2"], np.float32)
            bi = np.full(b.n, -1, np.int32); bd = np.full(b.n, 256, np.int32)
            keep.append((b, kb, sf, sg, jb["kf"]))
            w = arr[j]
            w.kf = jb["kf"]._h.value; w.pts = C.pointer(b); w.scale_factors = sf.ctypes.data; w.inv_sigma2 = None if sg is None else sg.ctypes.data
            w.nlevels = len(sf); w.th = float(jb.get("th", 3.0)); w.chi2 = 0 if sg is None else 1; w.max_dist = int(jb.get("max_dist", 50))
            w.best_idx = bi.ctypes.data; w.best_dist = bd.ctypes.data
            outs.append((bi, bd))
        _check(lib().orbx_frame_window_best_batch(arr, len(jobs)))
        return [(bi, bd, arr[j].nfound) for j, (bi, bd) in enumerate(outs)]

    def SearchByProjectionSim3Resident(self, kf, occupied, vpPoints, scaleFactors, th):
        """SearchByProjectionSim3 on a DeviceFrame, occupied (vpMatched[idx] != NULL) per call -> (match_kf, nmatches)"""
        oc = _occupied_for(occupied, kf, "SearchByProjectionSim3Resident")
        b, kb = self._points(vpPoints)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        out = np.full(kf.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_frame_search_by_projection_sim3(kf._h, None if oc is None else _p(oc), C.byref(b), _p(sf), len(sf), th, _p(out), C.byref(n)))
        return out, n.value

    def SearchBySim3Resident(self, kf1, kf2, pts12, pts21, scaleFactors1, scaleFactors2, th):
        """SearchBySim3 on two DeviceFrames: both directions in one launch -> (match12, nFound)"""
        p, kp = self._points(pts12); q, kq = self._points(pts21)
        s1 = np.ascontiguousarray(scaleFactors1, np.float32); s2 = np.ascontiguousarray(scaleFactors2, np.float32)
        out = np.full(kf1.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_frame_search_by_sim3(kf1._h, kf2._h, C.byref(p), C.byref(q), _p(s1), _p(s2), len(s1), th, _p(out), C.byref(n)))
        return out, n.value

    def SearchForInitialization(self, F1, F2, vbPrevMatched, windowSize=100):
        """SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize), src/ORBmatcher.cc:430-556
        -> (vnMatches12, nmatches, updated vbPrevMatched)"""
        a, ka = self._frame(F1); b, kb = self._frame(F2)
        xy = np.ascontiguousarray(vbPrevMatched, np.float32).reshape(-1, 2)
        out = np.full(a.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_search_for_initialization(self.device, C.byref(a), C.byref(b), _p(xy), int(windowSize), self.mfNNratio,
                                                    int(self.mbCheckOrientation), _p(out), C.byref(n)))
        new_xy = xy.copy(); m = out >= 0   # :544-546
        new_xy[m, 0] = kb["x"][out[m]]; new_xy[m, 1] = kb["y"][out[m]]
        return out, n.value, new_xy

    def SearchBySim3(self, pKF1, pKF2, pts12, pts21, scaleFactors1, scaleFactors2, th):
        """SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th), src/ORBmatcher.cc:1166-1394 -> (match12, nFound)"""
        a, ka = self._frame(pKF1); b, kb = self._frame(pKF2); p, kp = self._points(pts12); q, kq = self._points(pts21)
        s1 = np.ascontiguousarray(scaleFactors1, np.float32); s2 = np.ascontiguousarray(scaleFactors2, np.float32)
        out = np.full(a.n, -1, np.int32); n = C.c_int()
        _check(lib().orbx_search_by_sim3(self.device, C.byref(a), C.byref(b), C.byref(p), C.byref(q), _p(s1), _p(s2), len(s1), th,
                                         _p(out), C.byref(n)))
        return out, n.value

    def SearchForTriangulation(self, pKF1, pKF2, F12, ex, ey, scaleFactors2, levelSigma2_2, bOnlyStereo=False):
        a, ka = make_featset(pKF1); b, kb = make_featset(pKF2)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        sf = np.ascontiguousarray(scaleFactors2, np.float32); sg = np.ascontiguousarray(levelSigma2_2, np.float32)
        cap = max(a.n, 1)
        pairs = np.zeros((cap, 2), np.int32); n = C.c_int()
        _check(lib().orbx_search_for_triangulation(self.device, C.byref(a), C.byref(b), _p(F), ex, ey, _p(sf), _p(sg), len(sf),
                                                   int(bOnlyStereo), int(self.mbCheckOrientation), _p(pairs), cap, C.byref(n)))
        return pairs[:n.value].copy()


def UndistortKeyPoints(xy, fx, fy, cx, cy, distCoef, device=0):
    """Frame::UndistortKeyPoints (reference src/Frame.cc:470-515): cv::undistortPoints(mat, mat, mK, mDistCoef, Mat(), mK)"""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2); d = np.ascontiguousarray(distCoef, np.float32)
    out = np.zeros_like(xy)
    _check(lib().orbx_undistort_keypoints(device, _p(xy), len(xy), fx, fy, cx, cy, _p(d), len(d), _p(out)))
    return out


class Rectifier:
    """cv::remap(src, dst, M1, M2, INTER_LINEAR) with the CV_32FC1 maps of cv::initUndistortRectifyMap
    (reference Examples/Stereo/stereo_euroc.cc:103-104, :136-137), held on the device in OpenCV's fixed-point form."""

    def __init__(self, src_size, map_x, map_y, device=0):
        self._L = lib()
        mx = np.ascontiguousarray(map_x, np.float32); my = np.ascontiguousarray(map_y, np.float32)
        if mx.ndim != 2 or mx.shape != my.shape:
            raise OrbxError(-1, "map_x / map_y must be equal 2-D float32 arrays")
        h = C.c_void_p()
        _check(self._L.orbx_rectifier_create(device, int(src_size[0]), int(src_size[1]), mx.shape[1], mx.shape[0], _p(mx), _p(my), C.byref(h)))
        self._h = h; self.size = (mx.shape[1], mx.shape[0]); self.src_size = (int(src_size[0]), int(src_size[1]))

    def remap_batch_device(self, d_src, src_stride, src_pitch, batch, d_dst, dst_stride, dst_pitch, stream=None):
        _check(self._L.orbx_remap_batch_device(self._h, d_src, src_stride, src_pitch, batch, d_dst, dst_stride, dst_pitch, stream))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.orbx_rectifier_destroy(self._h); self._h = None
        except Exception:
            pass


def ComputeDistinctiveDescriptors(descriptor_sets, device=0):
    """Batched MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:266-340): one [n_i,32] uint8
    array per map point -> BestIdx per map point (-1 for an empty one)."""
    sets = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descriptor_sets]
    off = np.zeros(len(sets) + 1, np.int32)
    off[1:] = np.cumsum([len(d) for d in sets])
    flat = np.concatenate(sets) if len(sets) and off[-1] else np.zeros((0, 32), np.uint8)
    out = np.zeros(len(sets), np.int32)
    _check(lib().orbx_distinctive_descriptors(device, _p(flat), _p(off), len(sets), _p(out)))
    return out
