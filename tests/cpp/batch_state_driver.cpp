// batch_state_driver.cpp -- the batch states' registry and release (csrc/api_common.h: state_events, dev_array, state_own, state_release, state_free
// over csrc/ohgpu_internal.h's RunState) on the CPU, for tests/test_batch_state_cpu.py (built with -fsanitize=address,undefined
// -fno-sanitize-recover=all).  The device is stubbed: ctx_dev_alloc / ctx_dev_free are malloc / free over a set of the live blocks, an
// event is a heap byte, so a block or an event that nobody gives back is LeakSanitizer's to report and one given back twice is a
// failed check here.  Prints "ok" and returns 0 when every case holds.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>

#include "../../ohpipeline_amd/csrc/api_common.h"

using namespace ohgpu;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

namespace {
std::set<void*> g_blocks, g_events;
size_t g_allocs = 0, g_frees = 0, g_created = 0, g_destroyed = 0, g_drains = 0, g_uploads = 0;
size_t g_fail_event = ~(size_t)0, g_fail_alloc = ~(size_t)0;      // the call (counted from 0) that fails
}  // namespace

// ---- the library's side
namespace ohgpu {
int set_error(int code, const char*, ...) { return code; }
hipError_t ctx_dev_alloc(ohgpu_ctx*, void** p, size_t bytes)
{
    *p = nullptr;
    CHECK(bytes != 0);                                            // (dev_array allocates nothing for a zero count)
    if (g_allocs == g_fail_alloc) { g_fail_alloc = ~(size_t)0; return hipErrorOutOfMemory; }
    *p = malloc(bytes);
    g_blocks.insert(*p);
    g_allocs++;
    return hipSuccess;
}
void ctx_dev_free(ohgpu_ctx*, void* p)
{
    CHECK(p != nullptr);                                          // (state_release frees the blocks that exist)
    CHECK(g_blocks.erase(p) == 1);                                // ... each exactly once
    free(p);
    g_frees++;
}
}  // namespace ohgpu

// ---- the runtime's side
extern "C" {
hipError_t hipEventCreate(hipEvent_t* e)
{
    if (g_created == g_fail_event) { g_fail_event = ~(size_t)0; return hipErrorOutOfMemory; }
    *e = (hipEvent_t)malloc(1);
    g_events.insert(*e);
    g_created++;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    CHECK(g_events.erase(e) == 1);
    free(e);
    g_destroyed++;
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { g_drains++; return hipSuccess; }
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
{
    CHECK(kind == hipMemcpyHostToDevice && g_blocks.count(dst) == 1);
    memcpy(dst, src, bytes);
    g_uploads++;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stub"; }
}

namespace {

// A family's state and the batch that holds it by a pointer, released through state_free as ohgpu_batch_destroy's table does
struct DemoState : RunState {
    size_t n = 0;
    void* d_table = nullptr;
    void* d_results = nullptr;
    void* d_tiles = nullptr;
    void* d_list = nullptr; size_t list_cap = 0;      // a run's, grown on demand (FlacState::d_list)
};
struct Holder { DemoState* demo = nullptr; };
void demo_free(ohgpu_ctx* ctx, Holder* b) { state_free(ctx, b->demo); }
int demo_plan(ohgpu_ctx* ctx, DemoState& d, size_t n, size_t n_tiles)
{
    static const uint32_t table[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    const std::vector<uint16_t> tiles(n_tiles, 7);
    d.n = n;
    OHGPU_TRY(state_events(d, 5));
    OHGPU_TRY(dev_array(ctx, d, &d.d_table, 8, table));
    OHGPU_TRY(dev_array<uint64_t>(ctx, d, &d.d_results, n));
    OHGPU_TRY(dev_array(ctx, d, &d.d_tiles, n_tiles, tiles.data()));
    state_own(d, &d.d_list);
    return OHGPU_OK;
}
// flac_reserve's move: the block is freed and replaced in the middle of a run
void demo_grow(ohgpu_ctx* ctx, DemoState& d, size_t bytes)
{
    if (d.d_list && d.list_cap >= bytes) return;
    if (d.d_list) ctx_dev_free(ctx, d.d_list);
    d.d_list = nullptr; d.list_cap = 0;
    CHECK(ctx_dev_alloc(ctx, &d.d_list, bytes) == hipSuccess);
    d.list_cap = bytes;
}
struct Counts { size_t allocs, frees, created, destroyed, drains; };
Counts counts() { return Counts{g_allocs, g_frees, g_created, g_destroyed, g_drains}; }
void nothing_left() { CHECK(g_blocks.empty() && g_events.empty() && g_allocs == g_frees && g_created == g_destroyed); }

}  // namespace

int main()
{
    ohgpu_ctx ctx{};
    Holder b;

    // 1. fully built
    Counts c0 = counts();
    b.demo = new DemoState();
    CHECK(demo_plan(&ctx, *b.demo, 3, 5) == OHGPU_OK);
    CHECK(b.demo->n_events == 5 && b.demo->end_event() == b.demo->ev[4] && b.demo->end_event() != nullptr);
    CHECK(b.demo->d_table && b.demo->d_results && b.demo->d_tiles && !b.demo->d_list && b.demo->blocks.size() == 4);
    CHECK(((const uint32_t*)b.demo->d_table)[7] == 8 && ((const uint16_t*)b.demo->d_tiles)[4] == 7 && g_uploads == 2);
    demo_grow(&ctx, *b.demo, 64);
    CHECK(g_allocs - c0.allocs == 4 && g_created - c0.created == 5);
    demo_free(&ctx, &b);
    CHECK(!b.demo && g_frees - c0.frees == 4 && g_destroyed - c0.destroyed == 5 && g_drains - c0.drains == 1);
    nothing_left();

    // 2. some blocks null: zero counts allocate nothing and leave the pointer null, the list was never grown
    c0 = counts();
    b.demo = new DemoState();
    CHECK(demo_plan(&ctx, *b.demo, 0, 0) == OHGPU_OK);
    CHECK(b.demo->d_table && !b.demo->d_results && !b.demo->d_tiles && !b.demo->d_list && b.demo->blocks.size() == 4);
    CHECK(g_allocs - c0.allocs == 1);
    demo_free(&ctx, &b);
    CHECK(g_frees - c0.frees == 1 && g_destroyed - c0.destroyed == 5);
    nothing_left();

    // 3. a block replaced in the middle of a run, twice: the registry holds where the pointer lives, so the last one is freed, once
    c0 = counts();
    b.demo = new DemoState();
    CHECK(demo_plan(&ctx, *b.demo, 2, 1) == OHGPU_OK);
    demo_grow(&ctx, *b.demo, 64);
    void* const first = b.demo->d_list;
    demo_grow(&ctx, *b.demo, 32);
    CHECK(b.demo->d_list == first);
    demo_grow(&ctx, *b.demo, 4096);
    demo_grow(&ctx, *b.demo, 1 << 20);
    CHECK(g_allocs - c0.allocs == 6 && g_frees - c0.frees == 2 && g_blocks.size() == 4);
    demo_free(&ctx, &b);
    CHECK(g_frees - c0.frees == 6);
    nothing_left();

    // 4. released twice through state_free: the second call finds the pointer null
    c0 = counts();
    b.demo = new DemoState();
    CHECK(demo_plan(&ctx, *b.demo, 1, 1) == OHGPU_OK);
    demo_free(&ctx, &b);
    const Counts c1 = counts();
    demo_free(&ctx, &b);
    CHECK(counts().frees == c1.frees && counts().destroyed == c1.destroyed && counts().drains == c1.drains);
    nothing_left();

    // 5. a partly built batch: the state alone (no event, no block) ...
    c0 = counts();
    b.demo = new DemoState();
    demo_free(&ctx, &b);
    CHECK(g_frees == c0.frees && g_destroyed == c0.destroyed && g_drains - c0.drains == 1);
    // ... the third event refused: two exist, and every slot is looked at
    b.demo = new DemoState();
    g_fail_event = g_created + 2;
    CHECK(demo_plan(&ctx, *b.demo, 3, 5) == OHGPU_ERR_NOMEM);
    CHECK(g_created - c0.created == 2 && b.demo->ev[1] && !b.demo->ev[2] && b.demo->blocks.empty());
    demo_free(&ctx, &b);
    CHECK(g_destroyed - c0.destroyed == 2);
    nothing_left();
    // ... the second block refused: it is registered and null, the third was never reached
    c0 = counts();
    b.demo = new DemoState();
    g_fail_alloc = g_allocs + 1;
    CHECK(demo_plan(&ctx, *b.demo, 3, 5) == OHGPU_ERR_NOMEM);
    CHECK(b.demo->d_table && !b.demo->d_results && !b.demo->d_tiles && b.demo->blocks.size() == 2);
    demo_free(&ctx, &b);
    CHECK(g_frees - c0.frees == 1 && g_destroyed - c0.destroyed == 5);
    nothing_left();

    // 6. a state released by hand is left empty: releasing it again touches nothing
    DemoState d;
    CHECK(demo_plan(&ctx, d, 2, 2) == OHGPU_OK);
    state_release(&ctx, d);
    c0 = counts();
    state_release(&ctx, d);
    CHECK(g_frees == c0.frees && g_destroyed == c0.destroyed && !d.d_table && !d.ev[0]);
    nothing_left();

    // 7. state_free on a pointer that was never set: nothing is touched, the device is not drained
    c0 = counts();
    DemoState* none = nullptr;
    state_free(&ctx, none);
    CHECK(!none && g_frees == c0.frees && g_destroyed == c0.destroyed && g_drains == c0.drains);
    nothing_left();

    printf("ok\n");
    return 0;
}
