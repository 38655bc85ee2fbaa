// q3_prefix_cache.hip — the model's prefix cache (q3_prefix_cache.h) and its C ABI
#include "q3_prefix_cache.h"

static uint64_t block_key(uint64_t parent, const PrefixRegime* rg, const uint32_t* ids) {
    uint64_t h = 0xcbf29ce484222325ull ^ parent;                         // FNV-1a over (parent key | regime, ids)
    auto mix = [&](uint32_t w) { for (int i = 0; i < 4; ++i) { h ^= (w >> (8 * i)) & 0xffu; h *= 0x100000001b3ull; } };
    if (rg) for (int v : rg->v) mix((uint32_t)v);
    for (int i = 0; i < KV_PAGE_POS; ++i) mix(ids[i]);
    return h;
}
// the block behind `parent` (nullptr: block 0 of regime rg) that holds these ids; the caller holds c->mu
static PrefixBlock* find_block(PrefixCache* c, PrefixBlock* parent, const PrefixRegime& rg, const uint32_t* ids, uint64_t* key_out) {
    const uint64_t key = block_key(parent ? parent->key : 0, parent ? nullptr : &rg, ids);
    if (key_out) *key_out = key;
    auto range = c->blocks.equal_range(key);
    for (auto it = range.first; it != range.second; ++it) {
        PrefixBlock* b = it->second;
        if (b->parent != parent || (!parent && !(b->regime == rg))) continue;
        if (memcmp(b->ids, ids, sizeof b->ids) == 0) return b;
    }
    return nullptr;
}
static void drop_block(q3_model* m, PrefixCache* c, PrefixBlock* b) {      // the cache stops holding b's page; the caller holds c->mu
    auto range = c->blocks.equal_range(b->key);
    for (auto it = range.first; it != range.second; ++it) if (it->second == b) { c->blocks.erase(it); break; }
    if (b->parent) b->parent->children -= 1;
    std::vector<float*> one(1, b->page);
    m->kv_pool.give(one);
    delete b;
}
// the cache gives up every page. One that a row still holds stays that row's and goes back to the pool with it. The caller holds c->mu
static void drop_all(q3_model* m, PrefixCache* c) {
    std::vector<float*> pages;
    for (auto& kv : c->blocks) { pages.push_back(kv.second->page); delete kv.second; }
    c->blocks.clear();
    m->kv_pool.give(pages);
}
// the weights changed (q3_model_set_tensor, q3_model_mark_loaded, q3_model_finalize): cached K/V was computed with the old ones
void prefix_clear(q3_model* m) {
    PrefixCache* c = m->prefix;
    if (!c) return;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->blocks.empty()) drop_all(m, c);
}
// the least recently used leaf only the cache holds (never `keep`); the caller holds c->mu
static PrefixBlock* lru_leaf(q3_model* m, PrefixCache* c, const PrefixBlock* keep) {
    PrefixBlock* best = nullptr;
    std::lock_guard<std::mutex> gp(m->kv_pool.mu);      // one lock for the scan
    for (auto& kv : c->blocks) {
        PrefixBlock* b = kv.second;
        if (b == keep || b->children > 0 || (best && b->last_use >= best->last_use)) continue;
        if (m->kv_pool.is_shared_locked(b->page)) continue;
        best = b;
    }
    return best;
}

bool prefix_on(const q3_model* m) { return m->prefix && m->prefix->on.load(std::memory_order_relaxed) != 0; }

int prefix_peek(q3_model* m, const PrefixRegime& rg, const uint32_t* ids, int n_pages) {
    PrefixCache* c = m->prefix;
    std::lock_guard<std::mutex> g(c->mu);
    PrefixBlock* prev = nullptr; int k = 0;
    for (; k < n_pages; ++k) {
        PrefixBlock* b = find_block(c, prev, rg, ids + (size_t)k * KV_PAGE_POS, nullptr);
        if (!b) break;
        prev = b;
    }
    return k;
}
int prefix_acquire(q3_model* m, const PrefixRegime& rg, const uint32_t* ids, int n_pages, std::vector<float*>& out) {
    PrefixCache* c = m->prefix;
    std::lock_guard<std::mutex> g(c->mu);
    c->lookups += 1;
    PrefixBlock* prev = nullptr; int k = 0;
    for (; k < n_pages; ++k) {
        PrefixBlock* b = find_block(c, prev, rg, ids + (size_t)k * KV_PAGE_POS, nullptr);
        if (!b) break;
        m->kv_pool.share(b->page); out.push_back(b->page);
        b->last_use = ++c->clock; prev = b;
    }
    c->hit_positions += (long long)k * KV_PAGE_POS;
    return k;
}
void prefix_insert(q3_model* m, const PrefixRegime& rg, const uint32_t* ids, int n_pages, float* const* row_pages) {
    PrefixCache* c = m->prefix;
    std::lock_guard<std::mutex> g(c->mu);
    if (c->max_pages <= 0) return;
    PrefixBlock* prev = nullptr;
    for (int k = 0; k < n_pages; ++k) {
        uint64_t key = 0;
        PrefixBlock* b = find_block(c, prev, rg, ids + (size_t)k * KV_PAGE_POS, &key);
        if (!b) {
            while ((int)c->blocks.size() >= c->max_pages) {      // room: the LRU leaf nobody but the cache holds (not the one we hang off)
                PrefixBlock* v = lru_leaf(m, c, prev);
                if (!v) return;                                  // every block is in use or on this chain: the rest stays uncached
                drop_block(m, c, v); c->evictions += 1;
            }
            b = new PrefixBlock();
            b->key = key; b->parent = prev; b->regime = rg; b->page = row_pages[k];
            memcpy(b->ids, ids + (size_t)k * KV_PAGE_POS, sizeof b->ids);
            m->kv_pool.share(b->page);                           // the cache holds the row's page: no copy
            if (prev) prev->children += 1;
            c->blocks.emplace(key, b);
        }
        b->last_use = ++c->clock; prev = b;
    }
}
int prefix_evict(q3_model* m, int n_pages) {
    PrefixCache* c = m->prefix;
    if (!c) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    int n = 0;
    while (n < n_pages) {
        PrefixBlock* v = lru_leaf(m, c, nullptr);
        if (!v) break;
        drop_block(m, c, v); c->evictions += 1; ++n;
    }
    return n;
}
int prefix_reclaimable(q3_model* m) {
    PrefixCache* c = m->prefix;
    if (!c) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    int n = 0;
    std::lock_guard<std::mutex> gp(m->kv_pool.mu);
    for (auto& kv : c->blocks) n += m->kv_pool.is_shared_locked(kv.second->page) ? 0 : 1;
    return n;
}
hipError_t kv_take(q3_model* m, KvPool& pool, int n, std::vector<float*>& out) {
    hipError_t e = pool.take(n, out);
    while (e != hipSuccess && prefix_evict(m, 1) == 1) e = pool.take(n, out);      // one block at a time: no more than the request needs
    return e;
}

// ---- C ABI ----
extern "C" q3_status q3_model_prefix_cache(q3_model* m, int max_pages) {
    if (!m || m->device < 0 || !m->prefix) return set_err(Q3_INVALID_ARG, "q3_model_prefix_cache: no device model");
    if (max_pages < 0) return set_err(Q3_INVALID_ARG, "q3_model_prefix_cache: negative capacity");
    PrefixCache* c = m->prefix;
    std::lock_guard<std::mutex> g(c->mu);
    c->max_pages = max_pages; c->on.store(max_pages > 0 ? 1 : 0);
    if (max_pages == 0) { drop_all(m, c); return Q3_OK; }
    while ((int)c->blocks.size() > max_pages) {      // sized down: reclaimable blocks go, LRU leaf first; blocks in use stay for now
        PrefixBlock* v = lru_leaf(m, c, nullptr);
        if (!v) break;
        drop_block(m, c, v); c->evictions += 1;
    }
    return Q3_OK;
}
extern "C" q3_status q3_model_prefix_cache_info(q3_model* m, int* max_pages, int* pages_cached, int* pages_shared, long long* lookups,
                                                long long* hit_positions, long long* evictions) {
    if (!m || m->device < 0 || !m->prefix) return set_err(Q3_INVALID_ARG, "q3_model_prefix_cache_info: no device model");
    PrefixCache* c = m->prefix;
    std::lock_guard<std::mutex> g(c->mu);
    int shared = 0;
    {
        std::lock_guard<std::mutex> gp(m->kv_pool.mu);
        for (auto& kv : c->blocks) shared += m->kv_pool.is_shared_locked(kv.second->page) ? 1 : 0;
    }
    if (max_pages) *max_pages = c->max_pages;
    if (pages_cached) *pages_cached = (int)c->blocks.size();
    if (pages_shared) *pages_shared = shared;
    if (lookups) *lookups = c->lookups;
    if (hit_positions) *hit_positions = c->hit_positions;
    if (evictions) *evictions = c->evictions;
    return Q3_OK;
}
extern "C" q3_status q3_session_prefix_info(q3_session* s, int b, int* reused_positions) {
    if (!s || b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "q3_session_prefix_info: bad sequence index");
    if (!s->prefilled) return set_err(Q3_INVALID_ARG, "q3_session_prefix_info: session not prefilled");
    if (reused_positions) *reused_positions = s->seq[(size_t)b].reused;
    return Q3_OK;
}
