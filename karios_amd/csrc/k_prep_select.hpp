// The parts of the radix select that its two users compile: k_prep.hip (km_order_statistics: every pixel of a raster) and k_report.hip
// (km_display_range: the pixels a predicate keeps).  The key mapping, the run-merged LDS add and the one-workgroup kernel that picks,
// after each pass, the bin of every rank wanted.  Each translation unit gets a copy of its own (unnamed namespace): the instantiations
// of one do not depend on the other.
#pragma once
#include "k_prep.hpp"

namespace {

constexpr int kSelThreads = 256;
constexpr int kSelMaxBlocks = 2048;
constexpr unsigned kNone = 0xFFFFFFFFu;   // no bin: a pixel left out, a lane past the end, an unused prefix slot

// float32 bits -> uint32 whose unsigned order is the numeric order (-0.0 directly below +0.0)
__device__ __forceinline__ unsigned key_of(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }

// One LDS add per run of equal bins across the wave's lanes instead of one per lane.  Natural rasters put neighbouring pixels into the
// same coarse bin, so a plain atomic per lane serialises up to 64 adds on one LDS address; a run head adds the run's length once.
// Every lane of the wave must call this (it shuffles and ballots).
__device__ __forceinline__ void lds_add_runs(unsigned *h, unsigned idx)
{
    const unsigned lane = __lane_id();
    const unsigned prev = __shfl_up(idx, 1);
    const bool head = lane == 0 || prev != idx;
    const unsigned long long heads = __ballot(head);
    if (head && idx != kNone) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const unsigned len = above ? (unsigned)__ffsll((unsigned long long)above) : 64u - lane;
        atomicAdd(&h[idx], len);
    }
}

// After pass LEVEL: for every rank wanted, the bin of its slot's histogram that holds it and the rank inside that bin; the bins become
// the (distinct) prefixes of the next pass, or, after pass 3, the keys themselves.  One workgroup.
// VI32 (k_report.hip, float32 rasters): the virtual index as numpy computes it for a float32 array, float32(n - 1) * float32(q).
template <int LEVEL, bool VI32 = false>
__global__ __launch_bounds__(256) void select_pick_kernel(kp_state *__restrict__ st, kp_q4 q, int n_q)
{
    constexpr int NB = LEVEL == 1 ? KP_NB1 : KP_NB23, PER = NB / 256;
    __shared__ unsigned long long part[256];
    __shared__ unsigned long long s_rem[KP_MAX_RANKS];
    __shared__ unsigned s_bin[KP_MAX_RANKS];
    __shared__ int s_slot[KP_MAX_RANKS];
    __shared__ int s_nr;
    const int tid = threadIdx.x;

    if (LEVEL == 1) {
        unsigned long long s = 0;
        for (int i = 0; i < PER; i++) s += st->hist1[tid * PER + i];
        part[tid] = s;
        __syncthreads();
        if (tid == 0) {
            unsigned long long n = 0;
            for (int i = 0; i < 256; i++) n += part[i];
            st->n = (long long)n;
            int nr = 0;
            if (n > 0) {
                for (int j = 0; j < n_q; j++) {
                    const double vi = VI32 ? (double)__fmul_rn((float)(n - 1), (float)q.q[j])
                                           : (double)(n - 1) * q.q[j];   // numpy's virtual index of the 'linear' method
                    double f = floor(vi);
                    f = f < 0.0 ? 0.0 : f;
                    unsigned long long r0 = (unsigned long long)f;
                    if (r0 > n - 1) r0 = n - 1;
                    const unsigned long long r1 = r0 + 1 < n ? r0 + 1 : n - 1;
                    st->vi[j] = vi;
                    s_rem[nr] = r0; s_slot[nr] = 0; nr++;
                    s_rem[nr] = r1; s_slot[nr] = 0; nr++;
                }
            }
            s_nr = nr;
        }
    } else if (tid == 0) {
        const int nr = st->n_ranks;
        for (int r = 0; r < nr; r++) { s_rem[r] = st->rank_rem[r]; s_slot[r] = st->rank_slot[r]; }
        s_nr = nr;
    }
    __syncthreads();
    const int nr = s_nr;

    for (int r = 0; r < nr; r++) {
        const unsigned long long *hist = LEVEL == 1 ? st->hist1 : LEVEL == 2 ? st->hist2[s_slot[r]] : st->hist3[s_slot[r]];
        const unsigned long long rem = s_rem[r];
        unsigned long long cnt[PER], sum = 0;
        for (int i = 0; i < PER; i++) { cnt[i] = hist[tid * PER + i]; sum += cnt[i]; }
        __syncthreads();                       // (the previous round's readers of part[] are done)
        part[tid] = sum;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {    // inclusive scan of the 256 partial sums
            const unsigned long long add = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        unsigned long long below = part[tid] - sum;
        if (below <= rem && rem < below + sum) {   // exactly one thread: the total of a slot's histogram exceeds every rank kept in it
            int b = 0;
            for (int i = 0; i < PER; i++) {
                if (rem < below + cnt[i]) { b = i; break; }
                below += cnt[i];
            }
            s_bin[r] = (unsigned)(tid * PER + b);
            s_rem[r] = rem - below;
        }
    }
    __syncthreads();

    if (tid == 0) {
        unsigned np[KP_MAX_RANKS], slots[KP_MAX_RANKS];
        int slot_of[KP_MAX_RANKS], ns = 0;
        for (int r = 0; r < nr; r++) np[r] = LEVEL == 1 ? s_bin[r] : (st->prefix[s_slot[r]] << KP_BITS23) | s_bin[r];
        for (int r = 0; r < nr; r++) {
            int s = 0;
            while (s < ns && slots[s] != np[r]) s++;
            if (s == ns) slots[ns++] = np[r];
            slot_of[r] = s;
        }
        for (int s = 0; s < KP_MAX_RANKS; s++) st->prefix[s] = s < ns ? slots[s] : kNone;
        for (int r = 0; r < nr; r++) { st->rank_slot[r] = slot_of[r]; st->rank_rem[r] = s_rem[r]; }
        st->n_slots = ns;
        st->n_ranks = nr;
        if (LEVEL == 3)
            for (int j = 0; 2 * j + 1 < nr; j++) {
                st->v0[j] = (double)value_of(np[2 * j]);
                st->v1[j] = (double)value_of(np[2 * j + 1]);
            }
    }
}

}  // namespace
