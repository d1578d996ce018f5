// devbuf_main.cpp -- koifish_amd/host/kf_devbuf.hpp without a device (tests/test_devbuf_cpu.py builds it with AddressSanitizer + UBSan and runs it): the four ABI
// functions the header calls are defined here over host malloc, with a record of the live blocks, the ctx each was allocated with, and a countdown that makes the
// n-th allocation from now return KF_OUTOF_GPUMEMORY.  Exit 0 = every check held and no block is live.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../koifish_amd/host/kf_devbuf.hpp"

struct kf_ctx {
    int id;
};
static std::map<void*, std::pair<kf_ctx*, bool>> g_live;  // block -> {its ctx, came from kf_tp_alloc}
static int g_fail_in = 0;                                 // > 0: that many allocations from now, one is refused
static int g_frees = 0, g_wrong_ctx = 0, g_checks = 0, g_failed = 0;

static int stand_in_alloc(kf_ctx* c, size_t bytes, void** out, bool uncached) {
    if (!c || !out) return KF_INVALID_ARGS;
    if (g_fail_in > 0 && --g_fail_in == 0) return KF_OUTOF_GPUMEMORY; /* *out left as it was, like hipMalloc */
    *out = malloc(bytes ? bytes : 16);
    g_live[*out] = {c, uncached};
    return KF_OK;
}
extern "C" {
int kf_malloc(kf_ctx* c, size_t bytes, void** out) { return stand_in_alloc(c, bytes, out, false); }
int kf_tp_alloc(kf_ctx* c, size_t bytes, void** out) { return bytes ? stand_in_alloc(c, bytes, out, true) : KF_INVALID_ARGS; }
int kf_free(kf_ctx* c, void* p) {
    if (!p) return KF_OK;
    auto it = g_live.find(p);
    if (it == g_live.end()) return g_failed++, printf("kf_free of a block that is not live\n"), KF_INVALID_ARGS;
    g_frees++;
    if (it->second.first != c) g_wrong_ctx++;
    g_live.erase(it);
    free(p);
    return KF_OK;
}
int kf_memset(kf_ctx* c, void* p, int v, size_t bytes) {
    if (!c || g_live.find(p) == g_live.end()) return KF_INVALID_ARGS;
    memset(p, v, bytes);
    return KF_OK;
}
}

#define CHECK(cond)                                                          \
    do {                                                                     \
        g_checks++;                                                          \
        if (!(cond)) g_failed++, printf("line %d: %s\n", __LINE__, #cond);   \
    } while (0)

using koifish::DevBuf;
static kf_ctx A{1}, B{2};
static bool live(const void* p) { return g_live.count(const_cast<void*>(p)) == 1; }

// the pattern of kf_host.cpp's sets: Alloc fills a fresh object, the holder move-assigns it only when every member succeeded
struct Two {
    DevBuf<int8_t> q;
    DevBuf<float> step;
    int rows = 0;
    int Alloc(kf_ctx* c, int n) {
        if (int rc = q.Alloc(c, (size_t)n * 64)) return rc;
        if (int rc = step.AllocFilled(c, (size_t)n * 4)) return rc;
        rows = n;
        return KF_OK;
    }
};
struct Three {
    DevBuf<int32_t> a, b, c;
    int Alloc(kf_ctx* ctx, int n) {
        if (int rc = a.AllocFilled(ctx, (size_t)n * 16, 0)) return rc;
        if (int rc = b.AllocFilled(ctx, (size_t)n * 4, 0xff)) return rc;
        return c.AllocUncached(ctx, (size_t)n * 4);
    }
};
template <class Set>
static int grow(Set& held, kf_ctx* c, int n) {
    Set fresh;
    if (int rc = fresh.Alloc(c, n)) return rc;
    held = std::move(fresh);
    return KF_OK;
}

static void single_buffer() {
    {
        DevBuf<> e; /* an empty buffer frees nothing */
        CHECK(!e && e.get() == nullptr && e.bytes() == 0);
        e.Free();
    }
    CHECK(g_frees == 0 && g_live.empty());
    {
        DevBuf<int32_t> b;
        CHECK(b.Alloc(&A, 40) == KF_OK && b && b.bytes() == 40 && live(b) && g_live.size() == 1);
        int32_t* first = b;
        CHECK(b + 3 == first + 3); /* the implicit pointer view */
        CHECK(b.Alloc(&B, 80) == KF_OK && !live(first) && live(b) && g_live.size() == 1 && b.bytes() == 80); /* Alloc over a held block frees the old one */
        CHECK(b.AllocFilled(&A, 12, 0xff) == KF_OK && b[0] == -1 && b[2] == -1);
        CHECK(b.AllocFilled(&A, 12) == KF_OK && b[0] == 0 && b[2] == 0);
        g_fail_in = 1;
        CHECK(b.Alloc(&A, 16) == KF_OUTOF_GPUMEMORY && !b && b.get() == nullptr && b.bytes() == 0 && g_live.empty()); /* a failed Alloc: empty, never dangling */
        CHECK(b.Alloc(&B, 16) == KF_OK); /* and the same call can be made again */
    }
    CHECK(g_live.empty()); /* the end of scope leaves nothing */
    {
        DevBuf<uint8_t> u;
        CHECK(u.AllocUncached(&A, 64) == KF_OK && live(u) && g_live[u.get()].second); /* through the kf_tp_alloc stand-in */
        DevBuf<uint8_t> c;
        CHECK(c.Alloc(&A, 64) == KF_OK && !g_live[c.get()].second);
        CHECK(u.AllocUncached(&A, 0) == KF_INVALID_ARGS && !u);
    }
    CHECK(g_live.empty());
}

static void moves() {
    DevBuf<float> a, b;
    CHECK(a.Alloc(&A, 32) == KF_OK && b.Alloc(&B, 64) == KF_OK);
    float *pa = a, *pb = b;
    DevBuf<float> c(std::move(a)); /* move construction: transfers, empties the source */
    CHECK(c.get() == pa && c.bytes() == 32 && !a && a.bytes() == 0 && live(pa) && g_live.size() == 2);
    c = std::move(b); /* move assignment: frees the target's old block (with ITS ctx), takes the source's */
    CHECK(c.get() == pb && c.bytes() == 64 && !b && !live(pa) && live(pb) && g_live.size() == 1);
    DevBuf<float>& self = c;
    c = std::move(self); /* self-move is harmless */
    CHECK(c.get() == pb && c.bytes() == 64 && live(pb));
    c = DevBuf<float>(); /* an empty source empties the target */
    CHECK(!c && g_live.empty());
}

template <class Set>
static void set_commits_whole(int members, std::vector<const void*> (*blocks)(const Set&)) {
    Set held;
    CHECK(grow(held, &A, 4) == KF_OK && (int)g_live.size() == members);
    const std::vector<const void*> before = blocks(held);
    unsigned char bits[sizeof(Set)];
    memcpy(bits, &held, sizeof(Set));
    for (int fail_at = 1; fail_at <= members; fail_at++) { /* the failure at each member in turn */
        g_fail_in = fail_at;
        CHECK(grow(held, &B, 8) == KF_OUTOF_GPUMEMORY);
        CHECK(memcmp(bits, &held, sizeof(Set)) == 0);  /* the held set is bit for bit what it was ... */
        CHECK((int)g_live.size() == members);          /* ... the partial fresh one is gone ... */
        for (const void* p : before) CHECK(live(p) && g_live[const_cast<void*>(p)].first == &A); /* ... and its blocks are still live */
    }
    CHECK(grow(held, &B, 8) == KF_OK && (int)g_live.size() == members); /* the same call, made again */
    for (const void* p : before) CHECK(!live(p));
}

int main() {
    single_buffer();
    moves();
    set_commits_whole<Two>(2, [](const Two& s) { return std::vector<const void*>{s.q.get(), s.step.get()}; });
    CHECK(g_live.empty());
    set_commits_whole<Three>(3, [](const Three& s) { return std::vector<const void*>{s.a.get(), s.b.get(), s.c.get()}; });
    CHECK(g_live.empty() && g_wrong_ctx == 0 && g_frees > 0); /* every free was handed the ctx of its allocation */
    printf("%d checks, %d failed, %d frees, %d with another ctx, %zu live blocks\n", g_checks, g_failed, g_frees, g_wrong_ctx, g_live.size());
    return g_failed == 0 && g_wrong_ctx == 0 && g_live.empty() ? 0 : 1;
}
