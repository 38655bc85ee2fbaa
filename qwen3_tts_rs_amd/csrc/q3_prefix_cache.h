// q3_prefix_cache.h — the model's prefix cache: prefilled K/V pages of VoiceDesign instructions, shared across requests
// (not part of the C ABI). No reference counterpart: the reference builds its cache per call (kv_cache.rs:234-310,
// talker.rs:585-627).
//
// Block k of a chain covers prompt positions [128k, 128k + 128) = one page of the f32 pool. Its key is
// hash(key of block k-1, the block's 128 token ids); the ids are stored and compared, and a block matches only behind the very
// parent block the walk came through, so a hash collision never aliases. Block 0 hangs off a REGIME: everything besides the
// token ids that decides the bits of a prompt position's K/V (which prefill kernels run and how they cut the prompt) — two
// requests share pages only inside one regime, which is what makes a hit invisible except in time.
//
// Holders: the cache is one holder of each cached page (KvPool::share), every row that linked it another. A block only the
// cache holds is RECLAIMABLE: the LRU leaf of those goes first when the cache is full, when the pool's limit would otherwise
// refuse a page (kv_take) and when the cache is sized down. Rows link chains from block 0 on, so the blocks rows hold are
// prefix-closed and every reclaimable block can be reached leaf by leaf.
// Lock order: PrefixCache::mu, then KvPool::mu, then KvBudget::mu.
#pragma once
#include "q3_engine.h"

struct PrefixRegime {
    int v[6] = {0, 0, 0, 0, 0, 0};
    bool operator==(const PrefixRegime& o) const { return memcmp(v, o.v, sizeof v) == 0; }
};
struct PrefixBlock {
    uint64_t key = 0; PrefixBlock* parent = nullptr; PrefixRegime regime;      // regime: compared on block 0 only
    uint32_t ids[KV_PAGE_POS]; float* page = nullptr;
    uint64_t last_use = 0; int children = 0;
};
struct PrefixCache {
    std::mutex mu;
    int max_pages = 0;                                   // 0 = off
    std::unordered_multimap<uint64_t, PrefixBlock*> blocks;
    uint64_t clock = 0;
    long long lookups = 0, hit_positions = 0, evictions = 0;
    std::atomic<int> on{0};                              // max_pages > 0, readable without the lock
    ~PrefixCache() { for (auto& kv : blocks) delete kv.second; }      // (the pages go with the pool's slabs)
};

Q3_HIDDEN bool prefix_on(const q3_model* m);
// blocks of the chain for `ids` that are present, at most n_pages (no holder is added, no statistics)
Q3_HIDDEN int prefix_peek(q3_model* m, const PrefixRegime& rg, const uint32_t* ids, int n_pages);
// the first min(n_pages, present) pages of the chain, each with one more holder (the calling row), appended to `out`
Q3_HIDDEN int prefix_acquire(q3_model* m, const PrefixRegime& rg, const uint32_t* ids, int n_pages, std::vector<float*>& out);
// after a prefill: the row's first n_pages pages become blocks where the chain has none yet (the cache becomes a holder)
Q3_HIDDEN void prefix_insert(q3_model* m, const PrefixRegime& rg, const uint32_t* ids, int n_pages, float* const* row_pages);
Q3_HIDDEN void prefix_clear(q3_model* m);                        // every block goes (the capacity stays): the weights changed
Q3_HIDDEN int prefix_evict(q3_model* m, int n_pages);            // up to n_pages reclaimable blocks go; how many went
Q3_HIDDEN int prefix_reclaimable(q3_model* m);                   // blocks only the cache holds
// KvPool::take that evicts reclaimable blocks before it gives up (the pool's limit, or the device, said no)
Q3_HIDDEN hipError_t kv_take(q3_model* m, KvPool& pool, int n, std::vector<float*>& out);
