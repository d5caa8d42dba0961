// group_stats.hip -- the three tables of -s / --stats (summary.rs:10-32) counted on the device from the per-haplotype consequence-id
// lists the decode left there (include/v2p_frontend.h part 4).  gfx950, wave64.
//
// One workgroup per haplotype list, everything it needs in LDS:
//   present   bitmap over transcript ranks: the list's groups (a group exists as soon as one id of the list splits to its transcript)
//   filter    one-hash bit filter over (rank, ref_pos) of every membership; a bit found set marks the rank in
//   suspect   bitmap over ranks: groups that MAY hold two members on one ref_pos -- a superset of those that do
//   keys      members of suspect groups, rank << 40 | mut_pos << 24 | list index: sorted, this is sort_alterations' stable order
//   bins      22 type counters
// Pass A sets `present` and finds poison ids.  Pass B inserts every membership (own group, and each extra whose group is present) into
// the filter.  Pass C counts the members of unsuspected groups by type -- their ref_pos are all distinct, so drop_replicate keeps them
// all and the order does not matter -- and collects the others into `keys`.  Those are sorted (bitonic, in LDS) and every group among
// them is walked by one thread that applies drop_replicate literally (vcf_ds.rs:387-420): all ref_pos distinct -> all stay; else
// consecutive members of equal identity collapse, and survivors != distinct ref_pos is the reference's panic.
// A list that does not fit (rank beyond the bitmap, more suspect members than `keys` holds, 2^24 ids or more) is REFUSED: flagged,
// nothing counted.  Nothing reaches global memory before the list is known to be clean, so a refused or aborting list leaves no trace
// in the tables.
#include "group_stats.h"

namespace v2p {
namespace {

enum : uint32_t { M_ERR = 22, M_ERR_CODE, M_REFUSE, M_NSORT, M_ABORT_RANK, M_NPRESENT };

__global__ __launch_bounds__(STATS_THREADS) void group_stats_kernel(const StatsArgs a)
{
    extern __shared__ unsigned long long lds_keys[];                   // [C], then the 32-bit arrays
    const uint32_t W = a.bitmap_words, F = a.filter_words, C = a.sort_capacity;
    uint32_t* present = reinterpret_cast<uint32_t*>(lds_keys + C);
    uint32_t* suspect = present + W;
    uint32_t* filter = suspect + W;
    uint32_t* misc = filter + F;                                       // [0, 22) type bins, then M_*
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t h = blockIdx.x;
    const uint64_t b = a.hap_begin[h];
    const uint64_t n64 = a.hap_begin[h + 1] - b;

    for (uint32_t i = tid; i < 2 * W + F + STATS_MISC_WORDS; i += STATS_THREADS) present[i] = 0u;
    __syncthreads();
    if (tid == 0) { misc[M_ABORT_RANK] = ~0u; if (n64 >= STATS_MAX_LIST) misc[M_REFUSE] = 1u; }
    __syncthreads();
    const uint32_t n = misc[M_REFUSE] ? 0u : uint32_t(n64);
    const uint32_t* L = a.ids + b;
    const uint32_t rank_cap = W * 32u;

    // ---- pass A: the groups of the list; poison ids ----
    for (uint32_t k = tid; k < n; k += STATS_THREADS) {
        const uint32_t id = L[k];
        if (id >= a.n_csq) { misc[M_ERR] = 1u; atomicMax(&misc[M_ERR_CODE], STATS_ERR_RANGE); continue; }
        const StatsRec r = a.rec[id];
        if (r.flags & 2u) misc[M_ERR] = 1u;
        if (r.rank != ~0u) {
            if (r.rank >= rank_cap) misc[M_REFUSE] = 1u;
            else atomicOr(&present[r.rank >> 5], 1u << (r.rank & 31u));
        }
    }
    __syncthreads();
    if (misc[M_ERR]) {
        if (tid == 0) atomicMin(&a.status[0], (unsigned long long)h << 32 | misc[M_ERR_CODE]);
        return;
    }
    if (misc[M_REFUSE]) {
        if (tid == 0) { a.refused[h] = 1u; atomicAdd(&a.status[1], 1ull); }
        return;
    }

    // ---- pass B: every membership into the (rank, ref_pos) filter; a bit found set makes the group suspect ----
    auto insert = [&](uint32_t rank, uint32_t ref_pos) {
        const uint32_t hsh = filter_hash(rank, ref_pos), bit = 1u << (hsh & 31u);
        if (atomicOr(&filter[(hsh >> 5) & (F - 1u)], bit) & bit) atomicOr(&suspect[rank >> 5], 1u << (rank & 31u));
    };
    for (uint32_t k = tid; k < n; k += STATS_THREADS) {
        const uint32_t id = L[k];
        const StatsRec r = a.rec[id];
        if (!(r.flags & 1u) || r.rank >= rank_cap) continue;           // Mutation::new failed: in no group's alts (vcf_ds.rs:360-362)
        insert(r.rank, r.pos >> 16);
        if (r.flags >> 16) {
            const uint32_t e1 = a.extra_begin[id + 1];
            for (uint32_t e = a.extra_begin[id]; e < e1; ++e) {
                const uint32_t x = a.extra[e];
                if (x < rank_cap && (present[x >> 5] >> (x & 31u) & 1u)) insert(x, r.pos >> 16);
            }
        }
    }
    __syncthreads();

    // ---- pass C: members of unsuspected groups counted by type, the others collected for the sort ----
    auto collect = [&](uint32_t rank, uint32_t mut_pos, uint32_t k) {
        const uint32_t slot = atomicAdd(&misc[M_NSORT], 1u);
        if (slot < C) lds_keys[slot] = (unsigned long long)rank << 40 | (unsigned long long)mut_pos << 24 | k;
    };
    for (uint32_t base = 0; base < n; base += STATS_THREADS) {         // whole waves stay in the loop: the own-group count is a ballot
        const uint32_t k = base + tid;
        uint32_t own_type = 0xFFu;
        if (k < n) {
            const uint32_t id = L[k];
            const StatsRec r = a.rec[id];
            if ((r.flags & 1u) && r.rank < rank_cap) {
                const uint32_t type = r.flags >> 8 & 0xFFu, mut_pos = r.pos & 0xFFFFu;
                if (suspect[r.rank >> 5] >> (r.rank & 31u) & 1u) collect(r.rank, mut_pos, k);
                else own_type = type;
                if (r.flags >> 16) {
                    const uint32_t e1 = a.extra_begin[id + 1];
                    for (uint32_t e = a.extra_begin[id]; e < e1; ++e) {
                        const uint32_t x = a.extra[e];
                        if (x >= rank_cap || !(present[x >> 5] >> (x & 31u) & 1u)) continue;
                        if (suspect[x >> 5] >> (x & 31u) & 1u) collect(x, mut_pos, k);
                        else atomicAdd(&misc[type], 1u);
                    }
                }
            }
        }
        unsigned long long rem = __ballot(own_type != 0xFFu);          // most lanes of a wave share one or two types: one add per type
        while (rem) {
            const int leader = __ffsll((long long)rem) - 1;
            const uint32_t t = __shfl(own_type, leader);
            const unsigned long long m = __ballot(own_type == t);
            if (lane == uint32_t(leader)) atomicAdd(&misc[t], uint32_t(__popcll(m)));
            rem &= ~m;
        }
    }
    __syncthreads();
    const uint32_t ns = misc[M_NSORT];
    if (ns > C) {
        if (tid == 0) { a.refused[h] = 1u; atomicAdd(&a.status[1], 1ull); }
        return;
    }

    // ---- suspect groups: sort by (rank, mut_pos, list order), then drop_replicate per group ----
    if (ns) {
        uint32_t P = 1u;
        while (P < ns) P <<= 1;
        for (uint32_t i = ns + tid; i < P; i += STATS_THREADS) lds_keys[i] = ~0ull;
        for (uint32_t size = 2; size <= P; size <<= 1)
            for (uint32_t stride = size >> 1; stride; stride >>= 1) {
                __syncthreads();
                for (uint32_t i = tid; i < P; i += STATS_THREADS) {
                    const uint32_t j = i ^ stride;
                    if (j > i) {
                        const unsigned long long x = lds_keys[i], y = lds_keys[j];
                        if ((x > y) == ((i & size) == 0u)) { lds_keys[i] = y; lds_keys[j] = x; }
                    }
                }
            }
        __syncthreads();
        for (uint32_t i = tid; i < ns; i += STATS_THREADS) {
            const uint32_t rank = uint32_t(lds_keys[i] >> 40);
            if (i && uint32_t(lds_keys[i - 1] >> 40) == rank) continue;    // one thread per group, at its first member
            uint32_t j = i + 1;
            while (j < ns && uint32_t(lds_keys[j] >> 40) == rank) ++j;
            auto rec_at = [&](uint32_t m) { return a.rec[L[uint32_t(lds_keys[m]) & (STATS_MAX_LIST - 1u)]]; };
            uint32_t n_unique = 0;
            for (uint32_t m = i; m < j; ++m) {
                const uint32_t rp = rec_at(m).pos >> 16;
                bool seen = false;
                for (uint32_t q = i; q < m && !seen; ++q) seen = (rec_at(q).pos >> 16) == rp;
                n_unique += seen ? 0u : 1u;
            }
            if (n_unique == j - i) {
                for (uint32_t m = i; m < j; ++m) atomicAdd(&misc[rec_at(m).flags >> 8 & 0xFFu], 1u);
                continue;
            }
            uint32_t survivors = 0, prev = 0;
            for (uint32_t m = i; m < j; ++m) {
                const uint32_t ident = rec_at(m).ident;
                if (m == i || ident != prev) ++survivors;
                prev = ident;
            }
            if (survivors != n_unique) { atomicMin(&misc[M_ABORT_RANK], rank); continue; }
            prev = 0;
            for (uint32_t m = i; m < j; ++m) {
                const StatsRec r = rec_at(m);
                if (m == i || r.ident != prev) atomicAdd(&misc[r.flags >> 8 & 0xFFu], 1u);
                prev = r.ident;
            }
        }
        __syncthreads();
        if (misc[M_ABORT_RANK] != ~0u) {
            if (tid == 0) atomicMin(&a.status[0], (unsigned long long)h << 32 | (misc[M_ABORT_RANK] + 1u));
            return;
        }
    }

    // ---- the list is clean: its counts join the tables ----
    uint32_t cnt = 0;
    for (uint32_t w = tid; w < W; w += STATS_THREADS) {
        uint32_t bits = present[w];
        cnt += uint32_t(__popc(bits));
        while (bits) {
            const uint32_t r = w * 32u + uint32_t(__ffs(int(bits)) - 1);
            atomicAdd(&a.per_transcript[r], 1ull);
            bits &= bits - 1u;
        }
    }
    if (cnt) atomicAdd(&misc[M_NPRESENT], cnt);
    __syncthreads();
    if (tid < STATS_TYPES && misc[tid]) atomicAdd(&a.per_type[uint64_t(h >> 1) * STATS_TYPES + tid], (unsigned long long)misc[tid]);
    if (tid == 32) {
        if (misc[M_NPRESENT]) atomicAdd(&a.per_proband[h >> 1], (unsigned long long)misc[M_NPRESENT]);
        if (ns) atomicAdd(&a.status[2], (unsigned long long)ns);
    }
}

}  // namespace

hipError_t launch_group_stats(const StatsArgs& a, hipStream_t st)
{
    if (!a.n_haps) return hipSuccess;
    const uint64_t lds = stats_lds_bytes(a.bitmap_words, a.filter_words, a.sort_capacity);
    if (!a.bitmap_words || !a.filter_words || (a.filter_words & (a.filter_words - 1)) || !a.sort_capacity ||
        (a.sort_capacity & (a.sort_capacity - 1)) || uint64_t(a.bitmap_words) * 32u > STATS_MAX_RANKS || lds > 160u * 1024u)
        return hipErrorInvalidValue;
    if (lds > 64u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(group_stats_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(group_stats_kernel, dim3(a.n_haps), dim3(STATS_THREADS), size_t(lds), st, a);
    return hipGetLastError();
}

}  // namespace v2p
