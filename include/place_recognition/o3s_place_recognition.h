/*
 * o3s_place_recognition.h — C ABI of the one-to-many place-recognition front end (same shared library, libo3dslam_icp_hip.so):
 * the body of the loop of PlaceRecognition::buildLoopClosureConstraints (O3S/src/PlaceRecognition.cpp:71-85) for ONE finished
 * submap against ALL its candidates at once.  The per-pair calls (o3s_feature_correspondences, o3s_submap_feature_correspondences,
 * o3s_submap_registration_ransac) are unchanged; these entries give, target by target, the same bits as those calls in a loop.
 *
 * Arithmetic contract (that of o3s_feature_correspondences, o3s_cloud_ops.h): the squared distance of two feature columns is the
 * fp64 running sum of squared differences in row order; the nearest column is found with strict `<` in ascending index, so the
 * lowest index wins among equals; a column with a NaN has no nearest column and is nobody's nearest column.  The targets are read
 * through a table of up to O3S_PLACE_MAX_TARGETS device pointers — nothing is concatenated — and no target sees another.
 * One launch finds the nearest column of every target for every source column, one the nearest source column of every target
 * column; the mutual filter (pair (i, ij[i]) kept when ji[ij[i]] == i), the fallback (a target with fewer than 3 ransac_n mutual
 * pairs takes every (i, ij[i]) with ij[i] >= 0 instead — decided per target, on the device) and the order-preserving compaction
 * run on the device too.  What reaches the host before the RANSAC is one small copy: the pair counts and the fallback flags.
 *
 * (The header lives in a directory of its own: include/ itself holds the headers of the first device-side ABI, one list.)
 * Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_PLACE_RECOGNITION_H
#define O3S_PLACE_RECOGNITION_H

#include <stdint.h>

#include "../o3s_registration.h"
#include "../o3s_submap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define O3S_PLACE_MAX_TARGETS 16

/* Host arrays: src_feat dim x n_src, tgt_feat[k] dim x n_tgt[k] (column-major: a column is a feature), 1 <= dim <= 264,
 * 1 <= K <= O3S_PLACE_MAX_TARGETS.  out_pairs: K slices of 2 x n_src int32; slice k (at out_pairs + 2 n_src k) holds the n_out[k]
 * pairs (source column, column of target k) of target k in ascending source column.  used_fallback: K flags, nullable.
 * A target without columns (n_tgt[k] == 0; its pointer may be NULL) gives 0 pairs and no fallback; n_src == 0 gives 0 pairs
 * everywhere.  K out of range, dim out of range, ransac_n < 0, a NULL array that is needed, K n_src or the targets' columns
 * together >= 2^31: O3S_ERR_BAD_ARGUMENT. */
int o3s_feature_correspondences_multi(int device, const double* src_feat, int64_t n_src, const double* const* tgt_feat,
                                      const int64_t* n_tgt, int32_t K, int32_t dim, int32_t mutual_filter, int32_t ransac_n,
                                      int32_t* out_pairs, int64_t* n_out, int32_t* used_fallback);

/* The same between the RESIDENT feature set of `source` and those of K target submaps on the same device, on the source's
 * stream: neither a feature set nor an index array leaves HBM.  out_pairs: K slices of 2 x features_size(source) int32 as above
 * (nullable when the source's feature set is empty).
 * Decided before any work is enqueued: K < 1 or K > O3S_PLACE_MAX_TARGETS, a NULL submap, a target on another device:
 * O3S_ERR_BAD_ARGUMENT; a submap without a feature set: O3S_ERR_NOT_INITIALIZED.  A target with an EMPTY feature set gives 0
 * pairs for that target; the others are unaffected. */
int o3s_submaps_feature_correspondences(const o3s_submap* source, const o3s_submap* const* targets, int32_t K,
                                        int32_t mutual_filter, int32_t ransac_n, int32_t* out_pairs, int64_t* n_out,
                                        int32_t* used_fallback);

/* RegistrationRANSACBasedOnFeatureMatching of `source` against each of K targets: the correspondences above, then the RANSAC of
 * o3s_registration.h ("RANSAC": the contract) of every target from its slice of the device pair buffer, one target after the
 * other on the source's stream — no pair is uploaded.  results[k] equals what o3s_submap_registration_ransac(source, targets[k])
 * gives, bit for bit.  inlier_correspondences (nullable): K slices of 2 x features_size(source) int32, slice k the winner's
 * inlier pairs of target k (results[k].correspondences of them); n_correspondences (nullable): K sizes of the correspondence
 * sets the RANSACs ran on.  Error rules as above; invalid params: O3S_ERR_BAD_ARGUMENT. */
int o3s_submaps_registration_ransac(const o3s_submap* source, const o3s_submap* const* targets, int32_t K,
                                    int32_t mutual_filter, const o3s_ransac_params* params, o3s_ransac_result* results,
                                    int32_t* inlier_correspondences, int64_t* n_correspondences);

#ifdef __cplusplus
}
#endif
#endif /* O3S_PLACE_RECOGNITION_H */
