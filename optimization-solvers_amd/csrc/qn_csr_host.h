// qn_csr_host.h -- pure-host CSR helpers of the two sparse objectives (qn_host_sparse_logistic.hip.h; the sparse quadratic's creation in
// qn_host_objective.hip.h, which keeps only its own validation texts): validation of a rows x cols pattern, the int32 copy the device keeps, the
// transpose by a counting sort, and the static cut of the rows over workgroups.  NO HIP include and no dependency on the library:
// tests/test_ref_sparse_logistic.py compiles it into a stand-alone program under the host sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace qn_csr {

// row_ptr[0] == 0, row_ptr[rows] == nnz, non-decreasing; every column inside [0, cols), strictly increasing within a row.  Nothing is read past
// row_ptr[rows] or col[nnz - 1].  false: *err says which rule and where.
template <class I>
static bool validate(size_t rows, size_t cols, size_t nnz, const I* rp, const I* ci, std::string* err) {
    if (rp[0] != 0) { *err = "row_ptr[0] must be 0"; return false; }
    if (rp[rows] < 0 || (uint64_t)rp[rows] != (uint64_t)nnz) { *err = "row_ptr[m] must be nnz"; return false; }
    for (size_t i = 0; i < rows; ++i) {
        if (rp[i + 1] < rp[i]) { *err = "row_ptr decreases at row " + std::to_string(i); return false; }
        if ((uint64_t)rp[i + 1] > (uint64_t)nnz) { *err = "row_ptr exceeds nnz at row " + std::to_string(i); return false; }
        for (size_t j = (size_t)rp[i]; j < (size_t)rp[i + 1]; ++j) {
            if (ci[j] < 0 || (uint64_t)ci[j] >= (uint64_t)cols) { *err = "a column of row " + std::to_string(i) + " is outside [0, n)"; return false; }
            if (j > (size_t)rp[i] && ci[j] <= ci[j - 1]) {
                *err = "the columns of row " + std::to_string(i) + " are not strictly increasing (unsorted or duplicate)";
                return false;
            }
        }
    }
    return true;
}

// the device's copy of a VALIDATED pattern: int32 whatever came in (nnz <= 2^31 - 1 and cols <= 2^30 were checked by the caller)
template <class I>
static void narrow(size_t rows, size_t nnz, const I* rp, const I* ci, std::vector<int>& rp32, std::vector<int>& ci32) {
    rp32.resize(rows + 1);
    ci32.assign(std::max<size_t>(nnz, 1), 0);
    for (size_t i = 0; i <= rows; ++i) rp32[i] = (int)rp[i];
    for (size_t j = 0; j < nnz; ++j) ci32[j] = (int)ci[j];
}

// the CSR of A' by a counting sort: its rows (A's columns) come out with strictly increasing columns (A's row numbers).  tc and tv hold at
// least one entry, as the device's arrays do.
static void transpose(size_t rows, size_t cols, const int* rp, const int* ci, const double* val, std::vector<int>& tp, std::vector<int>& tc,
                      std::vector<double>& tv) {
    const size_t nnz = (size_t)rp[rows];
    tp.assign(cols + 1, 0);
    for (size_t j = 0; j < nnz; ++j) tp[(size_t)ci[j] + 1]++;
    for (size_t c = 0; c < cols; ++c) tp[c + 1] += tp[c];
    tc.assign(std::max<size_t>(nnz, 1), 0);
    tv.assign(std::max<size_t>(nnz, 1), 0.0);
    std::vector<int> fill(tp.begin(), tp.end() - 1);
    for (size_t i = 0; i < rows; ++i)
        for (int j = rp[i]; j < rp[i + 1]; ++j) {
            const int k = fill[(size_t)ci[j]]++;
            tc[(size_t)k] = (int)i;
            tv[(size_t)k] = val[j];
        }
}

struct Cut {
    int G = 1;              // regular workgroups
    std::vector<int> start; // G + 1: workgroup w walks rows [start[w], start[w + 1])
    std::vector<int> longs; // the rows of more than long_row entries, in row order: one workgroup each, behind the regular ones
    int lanes = 1;          // the automatic lanes per row
};

// lanes per row from the mean row length: the largest power of two that is at most half of it (1 .. 64) -- SparseQuadratic's rule
static int auto_lanes(size_t rows, size_t nnz) {
    const double mean = (double)nnz / (double)rows;
    int L = 1;
    while (L < 64 && (double)(2 * L) <= 0.5 * mean) L *= 2;
    return L;
}

// SparseQuadratic's static cut: the prefix weight of a row is the nonzeros + rows in front of it, G = ceil(total / 4096) capped at maxg, and
// workgroup w starts at the first row whose prefix weight reaches total w / G
static Cut cut(size_t rows, const int* rp, int maxg, int long_row) {
    Cut c;
    const size_t nnz = (size_t)rp[rows], total = nnz + rows;
    c.G = (int)std::min<size_t>((size_t)maxg, std::max<size_t>(1, (total + 4095) / 4096));
    c.start.resize((size_t)c.G + 1);
    for (int w = 0; w <= c.G; ++w) {
        const uint64_t target = (uint64_t)total * (uint64_t)w / (uint64_t)c.G;
        size_t lo = 0, hi = rows; // the first row i with row_ptr[i] + i >= target
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if ((uint64_t)rp[mid] + mid >= target) hi = mid; else lo = mid + 1;
        }
        c.start[(size_t)w] = (int)lo;
    }
    c.start[0] = 0; c.start[(size_t)c.G] = (int)rows;
    for (size_t i = 0; i < rows; ++i)
        if (rp[i + 1] - rp[i] > long_row) c.longs.push_back((int)i);
    c.lanes = auto_lanes(rows, nnz);
    return c;
}

} // namespace qn_csr
