// pre3_own.h -- who owns device and pinned memory.  Host only: no HIP header, so a stand-alone host program can build it
// (tests/own_host_main.cpp) with its own definitions of the five seam functions below.
//   DevBlock / PinBlock   one block, grown on demand: reserve(need, cap, ..) frees the old block first, then allocates exactly `cap` bytes
//   BlockList             the blocks that live as long as their owner and never grow: allocated through dev() / pin(), which hand back a typed raw pointer
//   Group                 blocks of a list created together on first use: complete, or gone with every pointer that aliased them null
//   StageRing             two mapped pinned blocks used alternately, each written again only after its pull has announced itself
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "../../include/pre3.h"

namespace pre3 {

// ---- the seam: defined once over HIP (pre3_api.hip), where a failure also sets the error message; a PRE3_* status each.  The frees take the size
// for the live-block count (pre3_test_live_blocks).  own_dev_zero: stream == nullptr -> synchronous, else asynchronous on that (hipStream_t) stream.
int own_dev_alloc(void **p, size_t bytes);
void own_dev_free(void *p, size_t bytes);
int own_pin_alloc(void **p, size_t bytes, unsigned flags);
void own_pin_free(void *p, size_t bytes);
int own_dev_zero(void *p, size_t bytes, void *stream);
// own_pin_alloc's flags: hipHostMalloc's Default, Portable and Mapped under names a host program has too (pre3_api.hip asserts that they are equal)
constexpr unsigned PIN_DEFAULT = 0, PIN_PORTABLE = 1, PIN_MAPPED = 2;

// how a new device block is zeroed: not at all, synchronously, or on the owner's stream (one that does not synchronise with the null stream)
struct Zero {
    bool on; void *stream;
    static Zero none() { return Zero{ false, nullptr }; }
    static Zero sync() { return Zero{ true, nullptr }; }
    static Zero on_stream(void *st) { return Zero{ true, st }; }
};

struct DevBlock {
    void *p = nullptr; size_t bytes = 0;
    DevBlock() = default;
    DevBlock(DevBlock &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBlock &operator=(DevBlock &&o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~DevBlock() { release(); }
    void release() { if (p) own_dev_free(p, bytes); p = nullptr; bytes = 0; }
    // bytes >= need: nothing.  Otherwise the old block goes first (peak memory does not rise), then exactly `cap` bytes, zeroed by `z`; on failure the
    // block is empty.  *replaced (may be null): the pointer changed.  Whatever may still read the old block has been waited for by the caller.
    int reserve(size_t need, size_t cap, Zero z, bool *replaced = nullptr)
    {
        if (replaced) *replaced = false;
        if (bytes >= need) return PRE3_OK;
        release();
        int rc = own_dev_alloc(&p, cap);
        if (rc != PRE3_OK) { p = nullptr; return rc; }
        bytes = cap;
        if (z.on && (rc = own_dev_zero(p, cap, z.stream)) != PRE3_OK) { release(); return rc; }
        if (replaced) *replaced = true;
        return PRE3_OK;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct PinBlock {
    void *p = nullptr; size_t bytes = 0;
    PinBlock() = default;
    PinBlock(PinBlock &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    PinBlock &operator=(PinBlock &&o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~PinBlock() { release(); }
    void release() { if (p) own_pin_free(p, bytes); p = nullptr; bytes = 0; }
    int reserve(size_t need, size_t cap, unsigned flags, bool *replaced = nullptr)      // DevBlock::reserve's rules; pinned memory is never zeroed here
    {
        if (replaced) *replaced = false;
        if (bytes >= need) return PRE3_OK;
        release();
        const int rc = own_pin_alloc(&p, cap, flags);
        if (rc != PRE3_OK) { p = nullptr; return rc; }
        bytes = cap;
        if (replaced) *replaced = true;
        return PRE3_OK;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

// the fixed list: *out is the typed pointer the owner's launch sites keep using; the list frees in its destructor (or when it is assigned an empty one)
struct BlockList {
    std::vector<DevBlock> devs; std::vector<PinBlock> pins;
    template <typename T> int dev(T **out, size_t bytes, Zero z)
    {
        DevBlock b;
        const int rc = b.reserve(bytes, bytes, z);
        *out = rc == PRE3_OK ? static_cast<T *>(b.p) : nullptr;
        if (rc == PRE3_OK) devs.push_back(std::move(b));
        return rc;
    }
    template <typename T> int pin(T **out, size_t bytes, unsigned flags)
    {
        PinBlock b;
        const int rc = b.reserve(bytes, bytes, flags);
        *out = rc == PRE3_OK ? static_cast<T *>(b.p) : nullptr;
        if (rc == PRE3_OK) pins.push_back(std::move(b));
        return rc;
    }
};

// An all-or-nothing group on a list: allocate through the scope, then commit().  A scope that ends uncommitted releases what it allocated and nulls
// every pointer it handed out (alias() for pointers into a block of the group); the guard is set by commit() alone, behind the last allocation.
struct Group {
    struct Ptr { void *at; void (*null)(void *at); };          // a typed pointer of the owner's, and how to null it through its own type
    BlockList &list; bool &guard; size_t dev0, pin0; std::vector<Ptr> ptrs; bool committed = false;
    Group(BlockList &l, bool &g) : list(l), guard(g), dev0(l.devs.size()), pin0(l.pins.size()) {}
    Group(const Group &) = delete;
    Group &operator=(const Group &) = delete;
    template <typename T> void alias(T **p) { ptrs.push_back(Ptr{ p, [](void *at) { *static_cast<T **>(at) = nullptr; } }); }
    template <typename T> int dev(T **out, size_t bytes, Zero z) { alias(out); return list.dev(out, bytes, z); }
    template <typename T> int pin(T **out, size_t bytes, unsigned flags) { alias(out); return list.pin(out, bytes, flags); }
    void commit() { committed = true; guard = true; }
    ~Group()
    {
        if (committed) return;
        list.devs.resize(dev0); list.pins.resize(pin0);
        for (const Ptr &p : ptrs) p.null(p.at);
        guard = false;
    }
};

// Two mapped pinned blocks for host data on its way to the device.  The pull out of slot k announces itself in mailbox word base + k; `wait` returns
// once it has (a PRE3_* status).  acquire: a ring below `need` waits for every used slot, frees both blocks and allocates both at `cap`; then the
// slots alternate, a used one waited for first.  A wait that fails leaves the ring as it was; an allocation that fails leaves it empty.
struct StageRing {
    PinBlock blk[2]; bool used[2] = { false, false }; int next = 0, base = 0; size_t cap = 0; unsigned flags = 0;
    int (*wait)(void *ctx, int slot) = nullptr; void *wait_ctx = nullptr;
    int acquire(size_t need, size_t cap_new, void **host, int *slot)
    {
        if (cap < need) {
            for (int k = 0; k < 2; ++k)
                if (used[k]) { const int rc = wait(wait_ctx, base + k); if (rc != PRE3_OK) return rc; }
            for (int k = 0; k < 2; ++k) { blk[k].release(); used[k] = false; }
            cap = 0;
            for (int k = 0; k < 2; ++k) {
                const int rc = blk[k].reserve(cap_new, cap_new, flags);
                if (rc != PRE3_OK) { blk[0].release(); return rc; }
            }
            cap = cap_new;
        }
        const int k = next;
        if (used[k]) { const int rc = wait(wait_ctx, base + k); if (rc != PRE3_OK) return rc; }
        next ^= 1;
        *host = blk[k].p; *slot = k;
        return PRE3_OK;
    }
    void release(int slot) { used[slot] = true; }      // the pull of this slot has been queued
};

}  // namespace pre3
