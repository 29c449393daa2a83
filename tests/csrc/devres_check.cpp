// TEST HARNESS: the owners of the engine host's device resources (smoothxg_amd/csrc/poa_devres.h: DevBuf, DevEvent, DevStream,
// OutGuard) on counting stand-ins for the HIP calls they make.  Plain C++17, no HIP, no GPU: compile with g++ (the test also
// builds it with -fsanitize=address,undefined).  Never shipped.
//
//   devres_check   hipMalloc / hipFree are malloc / free with a table of the live blocks, events and streams are live entries of
//   a table each; freeing or destroying what is not in its table aborts (a double free, a destroy of a moved-from handle).  The
//   next N hipMalloc calls can be made to fail.  Every case ends with nothing alive; a case that fails says so on stderr and the
//   exit status is 1.  It prints one line per case: name, then hipMalloc calls, hipFree calls, and a figure of the case.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sxg_poa.h"

// --- the stand-ins ---------------------------------------------------------------------
typedef int hipError_t;
static const hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
typedef struct StandInEvent* hipEvent_t;
typedef struct StandInStream* hipStream_t;

static std::map<void*, size_t> live_blocks;
static size_t live_bytes = 0;
static std::set<void*> live_events, live_streams;
static long n_malloc = 0, n_free = 0, fail_mallocs = 0;
static std::string last_text;
static int last_code = 0;

static hipError_t hipMalloc(void** p, size_t bytes) {
    ++n_malloc;
    if (fail_mallocs > 0) { --fail_mallocs; return hipErrorOutOfMemory; }
    *p = malloc(bytes ? bytes : 1);
    if (!*p) abort();
    live_blocks[*p] = bytes;
    live_bytes += bytes;
    return hipSuccess;
}
static hipError_t hipFree(void* p) {
    ++n_free;
    auto it = live_blocks.find(p);
    if (it == live_blocks.end()) { fprintf(stderr, "hipFree of a pointer that is not alive\n"); abort(); }
    live_bytes -= it->second;
    live_blocks.erase(it);
    free(p);
    return hipSuccess;
}
static void* table_new(std::set<void*>& t) { void* q = malloc(1); if (!q) abort(); t.insert(q); return q; }
static void table_delete(std::set<void*>& t, void* q, const char* what) {
    if (!t.erase(q)) { fprintf(stderr, "%s of a handle that is not alive\n", what); abort(); }
    free(q);
}
static hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)table_new(live_events); return hipSuccess; }
static hipError_t hipEventDestroy(hipEvent_t e) { table_delete(live_events, e, "hipEventDestroy"); return hipSuccess; }
static hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (hipStream_t)table_new(live_streams); return hipSuccess; }
static hipError_t hipStreamDestroy(hipStream_t s) { table_delete(live_streams, s, "hipStreamDestroy"); return hipSuccess; }
static int fail(int code, const std::string& text) { last_code = code; last_text = text; return code; }

#include "../../smoothxg_amd/csrc/poa_devres.h"

// --- the cases -------------------------------------------------------------------------
static int bad = 0;
#define EXPECT(x) do { if (!(x)) { ++bad; fprintf(stderr, "%s: %s\n", case_name, #x); } } while (0)
static const char* case_name = "";
static long m0 = 0, f0 = 0;
static void begin(const char* name) { case_name = name; m0 = n_malloc; f0 = n_free; fail_mallocs = 0; last_text.clear(); last_code = 0; }
static void end(long figure) {
    EXPECT(live_blocks.empty()); EXPECT(live_bytes == 0); EXPECT(live_events.empty()); EXPECT(live_streams.empty());
    printf("%s %ld %ld %ld\n", case_name, n_malloc - m0, n_free - f0, figure);
}
static size_t grown(size_t bytes) { return bytes + bytes / 8 + 256; }

struct Plan {   // (as the engine's per-launch resources: buffers, a stream, two events)
    DevStream stream;
    DevEvent e0, e1;
    DevBuf arena, work;
};

static int holds_five_and_returns_early(bool early) {
    DevBuf a, b, c;
    DevEvent e;
    DevStream s;
    if (a.ensure(1000) || b.ensure(10) || c.ensure(100000)) return -1;
    if (e.create() != hipSuccess || s.create(0) != hipSuccess) return -1;
    if (live_blocks.size() != 3 || live_events.size() != 1 || live_streams.size() != 1) return -2;
    if (early) return 1;
    a.release();
    return 0;
}

struct Result { void* _owner; int n; };
static int results_freed = 0;
static void result_free(Result* r) { free(r->_owner); r->_owner = nullptr; r->n = 0; ++results_freed; }
static int fills_result(Result* out, bool fails) {
    out->_owner = malloc(16); out->n = 3;
    OutGuard<Result, result_free> guard(out);
    if (fails) return fail(SXG_E_NODEVICE, "a step failed");
    guard.dismiss();
    return SXG_OK;
}

int main() {
    begin("scope-exit");
    {
        DevBuf a;
        DevEvent e;
        DevStream s;
        EXPECT(a.ensure(4096) == SXG_OK && a.p && a.cap == grown(4096));
        EXPECT(e.create() == hipSuccess && (hipEvent_t)e != nullptr);
        EXPECT(s.create(0) == hipSuccess && (hipStream_t)s != nullptr);
        EXPECT(live_blocks.size() == 1 && live_bytes == grown(4096) && live_events.size() == 1 && live_streams.size() == 1);
    }
    end(0);

    begin("early-return");
    EXPECT(holds_five_and_returns_early(true) == 1);
    EXPECT(live_blocks.empty() && live_events.empty() && live_streams.empty());
    EXPECT(holds_five_and_returns_early(false) == 0);
    end(0);

    begin("ensure-grows");
    {
        DevBuf a;
        EXPECT(a.ensure(1000) == SXG_OK && a.cap == grown(1000));
        EXPECT(a.ensure(5000) == SXG_OK && a.cap == grown(5000));
        EXPECT(live_blocks.size() == 1 && live_bytes == grown(5000));   // (the old block went back before the new one came)
        EXPECT(n_free - f0 == 1);
        a.as<char>()[grown(5000) - 1] = 1;
    }
    end((long)grown(5000));

    begin("ensure-smaller");
    {
        DevBuf a;
        EXPECT(a.ensure(5000) == SXG_OK);
        void* const p = a.p;
        const long calls = n_malloc;
        EXPECT(a.ensure(100) == SXG_OK && a.ensure(5000) == SXG_OK && a.ensure(grown(5000)) == SXG_OK && a.ensure(0) == SXG_OK);
        EXPECT(n_malloc == calls && a.p == p && a.cap == grown(5000) && n_free == f0);
    }
    end(0);

    begin("first-malloc-fails");
    {
        DevBuf a;
        fail_mallocs = 1;
        EXPECT(a.ensure(3000) == SXG_OK && a.p && a.cap == 3000 && live_bytes == 3000);   // (the retry asks for exactly the bytes)
        EXPECT(n_malloc - m0 == 2 && last_text.empty());
        a.as<char>()[2999] = 1;
    }
    end(3000);

    begin("both-mallocs-fail");
    {
        DevBuf a;
        EXPECT(a.ensure(64) == SXG_OK);
        fail_mallocs = 2;
        EXPECT(a.ensure(123456) == SXG_E_NOMEM && a.p == nullptr && a.cap == 0);
        EXPECT(last_code == SXG_E_NOMEM && last_text == "hipMalloc failed for 123456 bytes");
        EXPECT(live_blocks.empty());   // (what it held before is gone, as a growing buffer's contents always are)
        EXPECT(a.ensure(64) == SXG_OK && a.cap == grown(64));   // and the buffer is usable again
    }
    end(0);

    begin("move-construct");
    {
        DevBuf a;
        DevEvent e;
        DevStream s;
        EXPECT(a.ensure(777) == SXG_OK && e.create() == hipSuccess && s.create(0) == hipSuccess);
        void* const p = a.p;
        const hipEvent_t ev = e;
        const hipStream_t st = s;
        DevBuf b(std::move(a));
        DevEvent e2(std::move(e));
        DevStream s2(std::move(s));
        EXPECT(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == grown(777));
        EXPECT((hipEvent_t)e == nullptr && (hipEvent_t)e2 == ev && (hipStream_t)s == nullptr && (hipStream_t)s2 == st);
        EXPECT(live_blocks.size() == 1 && live_events.size() == 1 && live_streams.size() == 1);
    }
    end(0);

    begin("move-assign");
    {
        DevBuf a, b;
        DevEvent e, e2;
        DevStream s, s2;
        EXPECT(a.ensure(100) == SXG_OK && b.ensure(200) == SXG_OK);
        EXPECT(e.create() == hipSuccess && e2.create() == hipSuccess && s.create(0) == hipSuccess && s2.create(0) == hipSuccess);
        void* const p = a.p;
        b = std::move(a);   // the target's own block, event and stream go back first
        e2 = std::move(e);
        s2 = std::move(s);
        EXPECT(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == grown(100));
        EXPECT(live_blocks.size() == 1 && live_bytes == grown(100) && live_events.size() == 1 && live_streams.size() == 1);
        DevBuf& self = b;
        b = std::move(self);
        EXPECT(b.p == p && live_blocks.size() == 1);
    }
    end(0);

    begin("vector-of-unique-ptr");
    {
        std::vector<std::unique_ptr<Plan>> plans;
        for (int i = 0; i < 5; ++i) {
            auto r = std::make_unique<Plan>();
            EXPECT(r->stream.create(0) == hipSuccess && r->e0.create() == hipSuccess && r->e1.create() == hipSuccess);
            EXPECT(r->arena.ensure(1000 * (size_t)(i + 1)) == SXG_OK);
            if (i & 1) EXPECT(r->work.ensure(40) == SXG_OK);
            plans.push_back(std::move(r));
        }
        {   // one that is dropped before it is complete, as when creating its second event fails
            auto r = std::make_unique<Plan>();
            EXPECT(r->stream.create(0) == hipSuccess && r->e0.create() == hipSuccess);
        }
        EXPECT(live_blocks.size() == 7 && live_events.size() == 10 && live_streams.size() == 5);
        plans.clear();
        EXPECT(live_blocks.empty() && live_events.empty() && live_streams.empty());
    }
    end(0);

    begin("release-twice");
    {
        DevBuf a;
        EXPECT(a.ensure(10) == SXG_OK);
        a.release();
        EXPECT(a.p == nullptr && a.cap == 0 && live_blocks.empty());
        a.release();
        EXPECT(n_free - f0 == 1);
        DevEvent e;
        EXPECT(e.create() == hipSuccess);
        e.destroy(); e.destroy();
        EXPECT(e.create() == hipSuccess && e.create() == hipSuccess && live_events.size() == 1);   // (create on a live one replaces it)
    }
    end(0);

    begin("guard-frees");
    {
        Result r{nullptr, 0};
        results_freed = 0;
        EXPECT(fills_result(&r, true) == SXG_E_NODEVICE && results_freed == 1 && r._owner == nullptr && r.n == 0);
        EXPECT(last_text == "a step failed");
    }
    end(results_freed);

    begin("guard-dismissed");
    {
        Result r{nullptr, 0};
        results_freed = 0;
        EXPECT(fills_result(&r, false) == SXG_OK && results_freed == 0 && r._owner != nullptr && r.n == 3);
        result_free(&r);   // (the caller's own free, as after a successful call)
        EXPECT(results_freed == 1);
    }
    end(results_freed - 1);

    if (bad) fprintf(stderr, "%d checks failed\n", bad);
    return bad ? 1 : 0;
}
