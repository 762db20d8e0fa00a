// own_host_main.cpp -- 3pre_amd/csrc/pre3_own.h on the host (tests/test_own_host.py builds this with -fsanitize=address,undefined).  The five seam
// functions are defined here over malloc: they count live blocks, log every call and fail the k-th allocation on request.  argv[1] names the case; the
// exit status is 0 when every check of the case held, and LeakSanitizer's report at exit is the leak check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "pre3_own.h"

using namespace pre3;

namespace {

struct Event { char what; void *p; size_t bytes; void *stream; unsigned flags; };      // 'A' / 'F' device, 'a' / 'f' pinned, 'Z' zero
std::vector<Event> g_log;
std::map<void *, size_t> g_live;
int g_fail_in = 0;              // > 0: the g_fail_in-th allocation from now fails
int g_failures = 0;

void check(bool ok, const char *what, int line)
{
    if (!ok) { printf("FAILED line %d: %s\n", line, what); ++g_failures; }
}
#define CHECK(cond) check((cond), #cond, __LINE__)

int fake_alloc(char what, void **p, size_t bytes, unsigned flags)
{
    if (g_fail_in > 0 && --g_fail_in == 0) { *p = nullptr; g_log.push_back(Event{ '!', nullptr, bytes, nullptr, flags }); return PRE3_E_NOMEM; }
    *p = malloc(bytes ? bytes : 1);
    g_live[*p] = bytes;
    g_log.push_back(Event{ what, *p, bytes, nullptr, flags });
    return PRE3_OK;
}
void fake_free(char what, void *p, size_t bytes)
{
    auto it = g_live.find(p);
    CHECK(it != g_live.end());                     // freed once, and only what was allocated
    if (it != g_live.end()) { CHECK(it->second == bytes); g_live.erase(it); }
    g_log.push_back(Event{ what, p, bytes, nullptr, 0 });
    free(p);
}
size_t count(char what) { size_t n = 0; for (const Event &e : g_log) n += e.what == what; return n; }

}  // namespace

namespace pre3 {
int own_dev_alloc(void **p, size_t bytes) { return fake_alloc('A', p, bytes, 0); }
void own_dev_free(void *p, size_t bytes) { fake_free('F', p, bytes); }
int own_pin_alloc(void **p, size_t bytes, unsigned flags) { return fake_alloc('a', p, bytes, flags); }
void own_pin_free(void *p, size_t bytes) { fake_free('f', p, bytes); }
int own_dev_zero(void *p, size_t bytes, void *stream)
{
    CHECK(g_live.count(p) == 1 && g_live[p] == bytes);
    memset(p, 0, bytes);
    g_log.push_back(Event{ 'Z', p, bytes, stream, 0 });
    return PRE3_OK;
}
}  // namespace pre3

namespace {

int fake_stream;                // (its address stands for a stream)

void case_reserve_within()
{
    DevBlock d; PinBlock h;
    CHECK(d.reserve(100, 128, Zero::sync()) == PRE3_OK && h.reserve(100, 128, PIN_MAPPED) == PRE3_OK);
    void *const dp = d.p, *const hp = h.p;
    g_log.clear();
    bool replaced = true;
    for (size_t need : { (size_t)0, (size_t)1, (size_t)100, (size_t)128 }) {
        CHECK(d.reserve(need, 4096, Zero::sync(), &replaced) == PRE3_OK && !replaced);
        CHECK(h.reserve(need, 4096, PIN_MAPPED, &replaced) == PRE3_OK && !replaced);
    }
    CHECK(g_log.empty());                           // no allocator call, no zero call
    CHECK(d.p == dp && h.p == hp && d.bytes == 128 && h.bytes == 128);
}

void case_reserve_grows()
{
    for (int policy = 0; policy < 3; ++policy) {    // none, synchronous, on a stream
        const Zero z = policy == 0 ? Zero::none() : (policy == 1 ? Zero::sync() : Zero::on_stream(&fake_stream));
        DevBlock d;
        CHECK(d.reserve(64, 64, z) == PRE3_OK);
        void *const old = d.p;
        g_log.clear();
        bool replaced = false;
        CHECK(d.reserve(65, 80, z, &replaced) == PRE3_OK && replaced);
        // the old block is freed before the new one is requested: [F old 64][A new 80]([Z new 80 stream])
        CHECK(g_log.size() == (policy == 0 ? 2u : 3u));
        CHECK(g_log[0].what == 'F' && g_log[0].p == old && g_log[0].bytes == 64);
        CHECK(g_log[1].what == 'A' && g_log[1].bytes == 80 && g_log[1].p == d.p);
        if (policy != 0) CHECK(g_log[2].what == 'Z' && g_log[2].p == d.p && g_log[2].bytes == 80 && g_log[2].stream == (policy == 2 ? &fake_stream : nullptr));
        CHECK(count('Z') == (policy == 0 ? 0u : 1u));
        CHECK(d.bytes == 80 && g_live.size() == 1);
    }
    PinBlock h;
    CHECK(h.reserve(10, 16, PIN_DEFAULT) == PRE3_OK);
    void *const old = h.p;
    g_log.clear();
    bool replaced = false;
    CHECK(h.reserve(17, 65536, PIN_PORTABLE, &replaced) == PRE3_OK && replaced);
    CHECK(g_log.size() == 2 && g_log[0].what == 'f' && g_log[0].p == old && g_log[1].what == 'a' && g_log[1].bytes == 65536 && g_log[1].flags == PIN_PORTABLE);
    CHECK(count('Z') == 0);
}

void case_failed_grow()
{
    DevBlock d; PinBlock h;
    CHECK(d.reserve(8, 8, Zero::sync()) == PRE3_OK && h.reserve(8, 8, PIN_DEFAULT) == PRE3_OK);
    bool replaced = true;
    g_fail_in = 1;
    CHECK(d.reserve(9, 16, Zero::sync(), &replaced) == PRE3_E_NOMEM && !replaced);
    CHECK(d.p == nullptr && d.bytes == 0);
    g_fail_in = 1;
    CHECK(h.reserve(9, 16, PIN_DEFAULT, &replaced) == PRE3_E_NOMEM && !replaced);
    CHECK(h.p == nullptr && h.bytes == 0);
    CHECK(g_live.empty());
    CHECK(d.reserve(9, 16, Zero::sync(), &replaced) == PRE3_OK && replaced && d.bytes == 16);
    CHECK(h.reserve(9, 16, PIN_DEFAULT, &replaced) == PRE3_OK && replaced && h.bytes == 16);
    CHECK(g_live.size() == 2);
}

void case_move()
{
    {
        DevBlock a;
        CHECK(a.reserve(32, 32, Zero::none()) == PRE3_OK);
        void *const p = a.p;
        DevBlock b(std::move(a));
        CHECK(a.p == nullptr && a.bytes == 0 && b.p == p && b.bytes == 32);
        DevBlock c;
        CHECK(c.reserve(8, 8, Zero::none()) == PRE3_OK);
        c = std::move(b);                           // c's own block goes, b is empty
        CHECK(b.p == nullptr && b.bytes == 0 && c.p == p && g_live.size() == 1);
        PinBlock h, h2;
        CHECK(h.reserve(8, 8, PIN_MAPPED) == PRE3_OK);
        h2 = std::move(h);
        CHECK(h.p == nullptr && h2.bytes == 8);
    }
    CHECK(g_live.empty());
    CHECK(count('F') == 2 && count('f') == 1);      // each block freed once (fake_free refuses a second time)
    {
        BlockList l;
        int32_t *x = nullptr; double *y = nullptr;
        CHECK(l.dev(&x, 40, Zero::sync()) == PRE3_OK && l.pin(&y, 80, PIN_DEFAULT) == PRE3_OK && x != nullptr && y != nullptr);
        for (int k = 0; k < 40; ++k) { void *q = nullptr; CHECK(l.dev(&q, 8, Zero::none()) == PRE3_OK); }      // (the vector's own moves)
        CHECK(g_live.size() == 42 && g_live.count(x) == 1 && g_live.count(y) == 1);
        l = BlockList();                            // how pre3_destroy releases
        CHECK(g_live.empty());
    }
}

struct Five { int32_t *a = nullptr; double *b = nullptr, *b_tail = nullptr; void *c = nullptr; unsigned char *d = nullptr; float *e = nullptr; bool ready = false; };
int five_ensure(BlockList &l, Five &f)
{
    if (f.ready) return PRE3_OK;
    Group g(l, f.ready);
    int rc;
    if ((rc = g.dev(&f.a, 16, Zero::sync())) != PRE3_OK) return rc;
    if ((rc = g.dev(&f.b, 64, Zero::none())) != PRE3_OK) return rc;
    f.b_tail = f.b + 4; g.alias(&f.b_tail);
    if ((rc = g.pin(&f.c, 32, PIN_MAPPED)) != PRE3_OK) return rc;
    if ((rc = g.dev(&f.d, 8, Zero::on_stream(&fake_stream))) != PRE3_OK) return rc;
    if ((rc = g.pin(&f.e, 24, PIN_DEFAULT)) != PRE3_OK) return rc;
    g.commit();
    return PRE3_OK;
}
void case_group()
{
    for (int k = 1; k <= 5; ++k) {
        BlockList l;
        int32_t *keep = nullptr;
        CHECK(l.dev(&keep, 4, Zero::none()) == PRE3_OK);      // an older block of the list is not the group's to release
        Five f;
        g_fail_in = k;
        CHECK(five_ensure(l, f) == PRE3_E_NOMEM);
        CHECK(g_live.size() == 1 && g_live.count(keep) == 1);
        CHECK(!f.ready && f.a == nullptr && f.b == nullptr && f.b_tail == nullptr && f.c == nullptr && f.d == nullptr && f.e == nullptr);
        CHECK(five_ensure(l, f) == PRE3_OK && f.ready);
        CHECK(g_live.size() == 6 && f.a && f.b && f.b_tail == f.b + 4 && f.c && f.d && f.e);
        g_log.clear();
        CHECK(five_ensure(l, f) == PRE3_OK && g_log.empty());
    }
    CHECK(g_live.empty());
}

struct FakeWait { std::vector<int> slots; int fail_slot = -1; };
int fake_wait(void *ctx, int slot)
{
    FakeWait *w = static_cast<FakeWait *>(ctx);
    w->slots.push_back(slot);
    return slot == w->fail_slot ? PRE3_E_STATE : PRE3_OK;
}
void ring_init(StageRing &r, FakeWait &w, int base) { r.base = base; r.flags = PIN_MAPPED; r.wait = fake_wait; r.wait_ctx = &w; }

void case_ring_alternation()
{
    for (int base : { 0, 2 }) {
        StageRing r; FakeWait w;
        ring_init(r, w, base);
        g_log.clear();
        void *host[6]; int slot[6];
        for (int i = 0; i < 6; ++i) {
            const size_t before = w.slots.size();
            CHECK(r.acquire(1000, 65536, &host[i], &slot[i]) == PRE3_OK);
            CHECK(slot[i] == (i & 1) && host[i] == r.blk[i & 1].p);
            if (i < 2) CHECK(w.slots.size() == before);                                         // a slot that was never released is not waited for
            else CHECK(w.slots.size() == before + 1 && w.slots.back() == base + (i & 1));
            r.release(slot[i]);
        }
        CHECK(g_log.size() == 2 && count('a') == 2 && r.cap == 65536 && g_log.back().bytes == 65536 && g_log.back().flags == PIN_MAPPED);
        // an acquired slot that is not released (its pull was never queued) is not waited for either
        StageRing q; FakeWait wq;
        ring_init(q, wq, base);
        void *h; int s;
        for (int i = 0; i < 4; ++i) CHECK(q.acquire(8, 8, &h, &s) == PRE3_OK && s == (i & 1));
        CHECK(wq.slots.empty());
    }
}

void case_ring_growth()
{
    StageRing r; FakeWait w;
    ring_init(r, w, 2);
    void *h; int s;
    CHECK(r.acquire(100, 128, &h, &s) == PRE3_OK); r.release(s);
    CHECK(r.acquire(100, 128, &h, &s) == PRE3_OK); r.release(s);
    void *const old0 = r.blk[0].p, *const old1 = r.blk[1].p;
    g_log.clear(); w.slots.clear();
    CHECK(r.acquire(129, 4096, &h, &s) == PRE3_OK);
    CHECK(w.slots.size() == 2 && w.slots[0] == 2 && w.slots[1] == 3);                           // both used: two waits, and none for the fresh slot
    CHECK(g_log.size() == 4 && g_log[0].what == 'f' && g_log[0].p == old0 && g_log[1].what == 'f' && g_log[1].p == old1);
    CHECK(g_log[2].what == 'a' && g_log[2].bytes == 4096 && g_log[3].what == 'a' && g_log[3].bytes == 4096);
    CHECK(r.cap == 4096 && s == 0 && h == r.blk[0].p && !r.used[0] && !r.used[1] && g_live.size() == 2);
}

void case_ring_failure()
{
    StageRing r; FakeWait w;
    ring_init(r, w, 0);
    void *h = nullptr; int s = -1;
    CHECK(r.acquire(100, 128, &h, &s) == PRE3_OK); r.release(s);
    CHECK(r.acquire(100, 128, &h, &s) == PRE3_OK); r.release(s);
    void *const p0 = r.blk[0].p, *const p1 = r.blk[1].p;
    // a failing wait in front of a growth, and in front of a plain turn: returned, the ring as it was
    for (size_t need : { (size_t)1000, (size_t)100 }) {
        w.fail_slot = need == 1000 ? 1 : 0;
        g_log.clear();
        CHECK(r.acquire(need, 4096, &h, &s) == PRE3_E_STATE);
        CHECK(g_log.empty() && r.blk[0].p == p0 && r.blk[1].p == p1 && r.cap == 128 && r.next == 0 && r.used[0] && r.used[1]);
    }
    w.fail_slot = -1;
    // a failing second allocation: capacity 0, nothing live; the next acquire recovers
    g_fail_in = 2;
    CHECK(r.acquire(1000, 4096, &h, &s) == PRE3_E_NOMEM);
    CHECK(r.cap == 0 && g_live.empty() && r.blk[0].p == nullptr && r.blk[1].p == nullptr);
    g_fail_in = 1;                                                                              // ... and a failing first one
    CHECK(r.acquire(1000, 4096, &h, &s) == PRE3_E_NOMEM);
    CHECK(r.cap == 0 && g_live.empty());
    w.slots.clear();
    CHECK(r.acquire(1000, 4096, &h, &s) == PRE3_OK);
    CHECK(r.cap == 4096 && g_live.size() == 2 && h == r.blk[s].p && w.slots.empty());
}

const struct { const char *name; void (*run)(); } CASES[] = {
    { "reserve_within", case_reserve_within }, { "reserve_grows", case_reserve_grows }, { "failed_grow", case_failed_grow }, { "move", case_move },
    { "group", case_group }, { "ring_alternation", case_ring_alternation }, { "ring_growth", case_ring_growth }, { "ring_failure", case_ring_failure },
};

}  // namespace

int main(int argc, char **argv)
{
    for (const auto &c : CASES) {
        if (argc > 1 && strcmp(argv[1], c.name) != 0) continue;
        g_log.clear(); g_fail_in = 0;
        c.run();
        CHECK(g_live.empty());                      // every owner of the case is gone: nothing is live
        CHECK(g_fail_in == 0);                      // every requested failure happened
        printf("%s %s\n", c.name, g_failures ? "FAILED" : "ok");
        return g_failures ? 1 : 0;
    }
    printf("no such case\n");
    return 2;
}
