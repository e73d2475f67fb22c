// facade_internal.h -- shared by the translation units of libmatchinglib_poselib_mi355x.so (not installed).
#pragma once
#include "mlpl_c.h"

// The calling thread's library context (created on first use on device $MLPL_DEVICE or 0).  Throws cv::Exception when no gfx950 device
// is usable: the drop-in has no CPU fallback.
mlpl_ctx *mlpl_facade_default_ctx();

// One draw from the stream poselib::setRansacSeed controls on the calling thread: the fixed seed, or the clock as the reference's estimators
// take it.
unsigned mlpl_facade_draw_seed();

// The process-wide pair of cv::RNG states of the reference's ARRSAC samplers (function-local statics there, shared by the essential-matrix and
// the homography estimator), held under its mutex for the lifetime of this object.
struct mlpl_facade_arrsac_rng_lock {
    mlpl_facade_arrsac_rng_lock();
    ~mlpl_facade_arrsac_rng_lock();
    uint64_t *state;
};
