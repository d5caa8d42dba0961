// group_csr.hip -- the grouped CSR of v2p_groups_build (csrc/host/group_muts.cpp) produced on the device from the per-haplotype
// consequence-id lists the decode left there (include/v2p_frontend.h part 5).  gfx950, wave64.
//
// One workgroup per haplotype list, launched twice as in the decode: a COUNT launch writes {groups, members} of every list, a small
// scan turns them into each list's bases, and the EMIT launch recomputes the list and writes the final arrays in place.  In LDS:
//   present   bitmap over transcript ranks: the list's groups (a group exists as soon as one id of the list splits to its transcript)
//   gprefix   exclusive popcount prefix of `present` per word: the slot of a group among the list's groups
//   filter    one-hash bit filter over (rank, ref_pos) of every membership; a bit found set marks the rank in
//   suspect   bitmap over ranks: groups that MAY hold two members on one ref_pos -- a superset of those that do
//   keys      EVERY mut_ok membership of the list, rank << 40 | mut_pos << 24 | list index: sorted (bitonic), this is the member order
//             of v2p_groups_build before drop_replicate: groups ascending, inside a group sort_alterations' stable order
//   dropped   one bit per key: the member goes in drop_replicate's dedup_by; dprefix its popcount prefix per word
// Only suspect groups pay drop_replicate's walk (vcf_ds.rs:387-420, applied literally by one thread per group); in the others all
// ref_pos are distinct and every member stays.  A group without a mut_ok member has no key: group_transcript and group_member_begin
// come from the bitmap, and an empty group's begin is the begin of the next group that has a key (a lower bound in the sorted keys).
// A list that does not fit (rank beyond the bitmap, more memberships than `keys` holds, 2^24 ids or more) is REFUSED: flagged, zero
// groups and members counted, nothing written.  An aborting list (id out of range, poison id, drop_replicate's abort) is reported
// through status[0] as in group_stats.hip and the emit launch does not run.
#include "group_csr.h"
#include "block_scan.hpp"

namespace v2p {
namespace {

enum : uint32_t { G_ERR, G_ERR_CODE, G_REFUSE, G_NKEYS, G_ABORT_RANK, G_SCAN /* GROUPS_THREADS / 64 words: block_excl_scan's scratch */ };
static_assert(G_SCAN + GROUPS_THREADS / 64 <= GROUPS_MISC_WORDS, "misc words");

// exclusive popcount prefixes of bits[0, n) into prefix[0, n); returns the total.  Every thread of the workgroup calls it.
__device__ uint32_t word_prefix(const uint32_t* bits, uint32_t* prefix, uint32_t n, uint32_t* scan, uint32_t tid)
{
    const uint32_t per = (n + GROUPS_THREADS - 1u) / GROUPS_THREADS;
    const uint32_t w0 = min(tid * per, n), w1 = min(w0 + per, n);
    uint32_t sum = 0;
    for (uint32_t w = w0; w < w1; ++w) sum += uint32_t(__popc(bits[w]));
    uint32_t total;
    uint32_t run = block_excl_scan<GROUPS_THREADS>(sum, scan, &total);
    for (uint32_t w = w0; w < w1; ++w) { prefix[w] = run; run += uint32_t(__popc(bits[w])); }
    __syncthreads();
    return total;
}

template <bool EMIT>
__global__ __launch_bounds__(GROUPS_THREADS) void group_csr_kernel(const GroupsArgs a)
{
    extern __shared__ unsigned long long lds_keys[];                   // [C], then the 32-bit arrays
    const uint32_t W = a.bitmap_words, F = a.filter_words, C = a.key_capacity, DW = (C + 31u) / 32u;
    uint32_t* present = reinterpret_cast<uint32_t*>(lds_keys + C);
    uint32_t* gprefix = present + W;
    uint32_t* suspect = gprefix + W;
    uint32_t* filter = suspect + W;
    uint32_t* dropped = filter + F;
    uint32_t* dprefix = dropped + DW;
    uint32_t* misc = dprefix + DW;
    const uint32_t tid = threadIdx.x;
    const uint32_t h = blockIdx.x;
    if (EMIT) {
        if (h == 0 && tid == 0) a.group_member_begin[a.n_groups] = a.n_members;
        if (a.refused[h]) return;
    }
    const uint64_t b = a.hap_begin[h];
    const uint64_t n64 = a.hap_begin[h + 1] - b;

    for (uint32_t i = tid; i < 3u * W + F + 2u * DW + GROUPS_MISC_WORDS; i += GROUPS_THREADS) present[i] = 0u;
    __syncthreads();
    if (tid == 0) { misc[G_ABORT_RANK] = ~0u; if (n64 >= STATS_MAX_LIST) misc[G_REFUSE] = 1u; }
    __syncthreads();
    const uint32_t n = misc[G_REFUSE] ? 0u : uint32_t(n64);
    const uint32_t* L = a.ids + b;
    const uint32_t rank_cap = W * 32u;
    // the ways out of a list that yields nothing: both launches leave the output arrays alone
    auto abort_list = [&](uint32_t reason) {
        if (!EMIT && tid == 0) {
            atomicMin(&a.status[0], (unsigned long long)h << 32 | reason);
            a.counts[2u * h] = 0u; a.counts[2u * h + 1u] = 0u;
        }
    };
    auto refuse_list = [&]() {
        if (!EMIT && tid == 0) {
            a.refused[h] = 1u; atomicAdd(&a.status[1], 1ull);
            a.counts[2u * h] = 0u; a.counts[2u * h + 1u] = 0u;
        }
    };

    // ---- pass A: the groups of the list; ids out of range, poison ids ----
    for (uint32_t k = tid; k < n; k += GROUPS_THREADS) {
        const uint32_t id = L[k];
        if (id >= a.n_csq) { misc[G_ERR] = 1u; atomicMax(&misc[G_ERR_CODE], STATS_ERR_RANGE); continue; }
        const StatsRec r = a.rec[id];
        if (r.flags & 2u) misc[G_ERR] = 1u;
        if (r.rank != ~0u) {
            if (r.rank >= rank_cap) misc[G_REFUSE] = 1u;
            else atomicOr(&present[r.rank >> 5], 1u << (r.rank & 31u));
        }
    }
    __syncthreads();
    if (misc[G_ERR]) { abort_list(misc[G_ERR_CODE]); return; }
    if (misc[G_REFUSE]) { refuse_list(); return; }
    const uint32_t n_groups = word_prefix(present, gprefix, W, misc + G_SCAN, tid);

    // ---- pass B: every membership into the (rank, ref_pos) filter; a bit found set makes the group suspect ----
    auto insert = [&](uint32_t rank, uint32_t ref_pos) {
        const uint32_t hsh = filter_hash(rank, ref_pos), bit = 1u << (hsh & 31u);
        if (atomicOr(&filter[(hsh >> 5) & (F - 1u)], bit) & bit) atomicOr(&suspect[rank >> 5], 1u << (rank & 31u));
    };
    // ---- and into the keys (own group, and each extra whose group is present) ----
    auto collect = [&](uint32_t rank, uint32_t mut_pos, uint32_t k) {
        const uint32_t slot = atomicAdd(&misc[G_NKEYS], 1u);
        if (slot < C) lds_keys[slot] = (unsigned long long)rank << 40 | (unsigned long long)mut_pos << 24 | k;
        else misc[G_REFUSE] = 1u;
    };
    for (uint32_t k = tid; k < n; k += GROUPS_THREADS) {
        if (*reinterpret_cast<volatile uint32_t*>(&misc[G_REFUSE])) break;     // over capacity already: the counter stays far from wrapping
        const uint32_t id = L[k];
        const StatsRec r = a.rec[id];
        if (!(r.flags & 1u) || r.rank >= rank_cap) continue;           // Mutation::new failed: in no group's alts (vcf_ds.rs:360-362)
        const uint32_t mut_pos = r.pos & 0xFFFFu, ref_pos = r.pos >> 16;
        insert(r.rank, ref_pos);
        collect(r.rank, mut_pos, k);
        if (r.flags >> 16) {
            const uint32_t e1 = a.extra_begin[id + 1];
            for (uint32_t e = a.extra_begin[id]; e < e1; ++e) {
                const uint32_t x = a.extra[e];
                if (x < rank_cap && (present[x >> 5] >> (x & 31u) & 1u)) { insert(x, ref_pos); collect(x, mut_pos, k); }
            }
        }
    }
    __syncthreads();
    if (misc[G_REFUSE]) { refuse_list(); return; }
    const uint32_t nk = misc[G_NKEYS];                                  // <= C

    // ---- sort by (rank, mut_pos, list order); then drop_replicate in every suspect group ----
    if (nk) {
        uint32_t P = 1u;
        while (P < nk) P <<= 1;
        for (uint32_t i = nk + tid; i < P; i += GROUPS_THREADS) lds_keys[i] = ~0ull;
        for (uint32_t size = 2; size <= P; size <<= 1)
            for (uint32_t stride = size >> 1; stride; stride >>= 1) {
                __syncthreads();
                for (uint32_t i = tid; i < P; i += GROUPS_THREADS) {
                    const uint32_t j = i ^ stride;
                    if (j > i) {
                        const unsigned long long x = lds_keys[i], y = lds_keys[j];
                        if ((x > y) == ((i & size) == 0u)) { lds_keys[i] = y; lds_keys[j] = x; }
                    }
                }
            }
        __syncthreads();
        for (uint32_t i = tid; i < nk; i += GROUPS_THREADS) {
            const uint32_t rank = uint32_t(lds_keys[i] >> 40);
            if (i && uint32_t(lds_keys[i - 1] >> 40) == rank) continue;    // one thread per group, at its first member
            if (!(suspect[rank >> 5] >> (rank & 31u) & 1u)) continue;      // all ref_pos distinct: all stay
            uint32_t j = i + 1;
            while (j < nk && uint32_t(lds_keys[j] >> 40) == rank) ++j;
            auto rec_at = [&](uint32_t m) { return a.rec[L[uint32_t(lds_keys[m]) & (STATS_MAX_LIST - 1u)]]; };
            uint32_t n_unique = 0;
            for (uint32_t m = i; m < j; ++m) {
                const uint32_t rp = rec_at(m).pos >> 16;
                bool seen = false;
                for (uint32_t q = i; q < m && !seen; ++q) seen = (rec_at(q).pos >> 16) == rp;
                n_unique += seen ? 0u : 1u;
            }
            if (n_unique == j - i) continue;
            uint32_t survivors = 0, prev = 0;
            for (uint32_t m = i; m < j; ++m) {
                const uint32_t ident = rec_at(m).ident;
                if (m == i || ident != prev) ++survivors;
                else atomicOr(&dropped[m >> 5], 1u << (m & 31u));
                prev = ident;
            }
            if (survivors != n_unique) atomicMin(&misc[G_ABORT_RANK], rank);
        }
        __syncthreads();
        if (misc[G_ABORT_RANK] != ~0u) { abort_list(misc[G_ABORT_RANK] + 1u); return; }
    }
    const uint32_t n_dropped = word_prefix(dropped, dprefix, (nk + 31u) / 32u, misc + G_SCAN, tid);
    const uint32_t n_members = nk - n_dropped;
    if (!EMIT) {
        if (tid == 0) { a.counts[2u * h] = n_groups; a.counts[2u * h + 1u] = n_members; }
        return;
    }

    // ---- the list is clean: its part of the three arrays ----
    const uint64_t gb = a.hap_group_begin[h], mb = a.hap_member_begin[h];
    auto survivors_before = [&](uint32_t i) {                          // among keys [0, i), i <= nk
        if (i >= nk) return n_members;
        return i - (dprefix[i >> 5] + uint32_t(__popc(dropped[i >> 5] & ((1u << (i & 31u)) - 1u))));
    };
    for (uint32_t i = tid; i < nk; i += GROUPS_THREADS) {
        if (dropped[i >> 5] >> (i & 31u) & 1u) continue;
        const uint64_t at = mb + survivors_before(i);
        if (at < a.n_members) a.member_ids[at] = L[uint32_t(lds_keys[i]) & (STATS_MAX_LIST - 1u)];
    }
    for (uint32_t w = tid; w < W; w += GROUPS_THREADS) {
        uint32_t bits = present[w];
        uint64_t at = gb + gprefix[w];
        while (bits) {
            const uint32_t r = w * 32u + uint32_t(__ffs(int(bits)) - 1);
            const unsigned long long want = (unsigned long long)r << 40;
            uint32_t lo = 0, hi = nk;                                  // the first key of rank >= r: where the group's members begin
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (lds_keys[mid] < want) lo = mid + 1u; else hi = mid;
            }
            if (at < a.n_groups) { a.group_transcript[at] = r; a.group_member_begin[at] = mb + survivors_before(lo); }
            ++at;
            bits &= bits - 1u;
        }
    }
}

// exclusive prefix sums of the lists' {groups, members}: one workgroup, a chunk of consecutive lists per thread
__global__ __launch_bounds__(GROUPS_THREADS) void group_csr_scan_kernel(const GroupsArgs a)
{
    __shared__ unsigned long long scratch[GROUPS_THREADS / 64];
    const uint32_t tid = threadIdx.x, n = a.n_haps;
    const uint32_t per = (n + GROUPS_THREADS - 1u) / GROUPS_THREADS;
    const uint32_t h0 = min(tid * per, n), h1 = min(h0 + per, n);
    unsigned long long g = 0, m = 0, g_total, m_total;
    for (uint32_t h = h0; h < h1; ++h) { g += a.counts[2u * h]; m += a.counts[2u * h + 1u]; }
    g = block_excl_scan<GROUPS_THREADS>(g, scratch, &g_total);
    m = block_excl_scan<GROUPS_THREADS>(m, scratch, &m_total);
    if (tid == 0) { a.hap_group_begin[n] = g_total; a.hap_member_begin[n] = m_total; }
    for (uint32_t h = h0; h < h1; ++h) {
        a.hap_group_begin[h] = g; a.hap_member_begin[h] = m;
        g += a.counts[2u * h]; m += a.counts[2u * h + 1u];
    }
}

hipError_t check_caps(const GroupsArgs& a, uint64_t& lds)
{
    lds = groups_lds_bytes(a.bitmap_words, a.filter_words, a.key_capacity);
    if (!a.bitmap_words || !a.filter_words || (a.filter_words & (a.filter_words - 1)) || !a.key_capacity ||
        (a.key_capacity & (a.key_capacity - 1)) || uint64_t(a.bitmap_words) * 32u > STATS_MAX_RANKS || lds > 160u * 1024u)
        return hipErrorInvalidValue;
    return hipSuccess;
}

template <bool EMIT>
hipError_t launch(const GroupsArgs& a, hipStream_t st)
{
    if (!a.n_haps) return hipSuccess;
    uint64_t lds = 0;
    hipError_t e = check_caps(a, lds);
    if (e != hipSuccess) return e;
    if (lds > 64u * 1024u) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(group_csr_kernel<EMIT>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(group_csr_kernel<EMIT>, dim3(a.n_haps), dim3(GROUPS_THREADS), size_t(lds), st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_groups_count(const GroupsArgs& a, hipStream_t st) { return launch<false>(a, st); }
hipError_t launch_groups_emit(const GroupsArgs& a, hipStream_t st) { return launch<true>(a, st); }

hipError_t launch_groups_scan(const GroupsArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(group_csr_scan_kernel, dim3(1), dim3(GROUPS_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace v2p
