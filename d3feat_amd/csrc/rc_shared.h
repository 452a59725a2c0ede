// RANSAC registration of every pair at every keypoint count (d3f_register_pairs_counts): what the two halves of the call share.
// registration.hip (rp_register_counts.h) owns the entry point, the nearest descriptors and the hypotheses; radius_neighbors.hip
// (nb_register_counts.h) owns everything that walks the cell grid, whose internals stay private to it: the stack of the blocks' xyz,
// the grid over it, the scoring of the hypotheses and the selection of the winner.
#pragma once
#include "common.h"

struct RcCounts {
    int k[D3F_REPEAT_COUNTS_MAX];     // strictly ascending
    int off[D3F_REPEAT_COUNTS_MAX];   // off[c] = k[0] + ... + k[c-1]
    int n, total;                     // total = sum of k
};

// what the hypotheses kernel leaves per (pair, count) -- lists of max_validation entries, (pair, count) = p * n + c
struct RcLists {
    const float* Tlist;      // f32[P, n, max_validation, 12]
    const int* itlist;       // i32[P, n, max_validation]
    const int* validations;  // i32[P, n]
    int* cnt;                // i32[P, n, max_validation]   scratch of the scoring
    unsigned long long* sd2; // u64[P, n, max_validation]
    int max_validation;
};
struct RcOut {
    float* T_out; int* inliers; unsigned long long* sumd2; int* best_iteration; int* nearest;   // nearest may be null
};

// bytes of the stack, its lengths and the grid over n_blocks blocks of at most `rows` rows
size_t nb_rc_workspace_bytes(int n_blocks, int rows);
// gather -> grid build -> score -> select on `stream`; `rows` = min(K, largest count)
int nb_rc_score_select(const float* kp, int n_blocks, int K, int ld, const int* count_dev, const int* pairs_dev, int P, const RcCounts& prm,
                       int rows, float radius, const RcLists& lists, const RcOut& out, void* workspace, size_t workspace_bytes,
                       hipStream_t stream);
