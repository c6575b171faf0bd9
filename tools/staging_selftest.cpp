// staging_selftest.cpp -- walks Staged (csrc/xsmm_staging.cpp) through its carving, copy-back and wait decision on plain malloc'ed
// memory, with stand-ins for the six functions it is built on. Host code only, meant for the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -Iinclude tools/staging_selftest.cpp
//       libxsmm-1_amd/csrc/xsmm_staging.cpp -o staging_selftest && ./staging_selftest
#include "../libxsmm-1_amd/csrc/xsmm_internal.hpp"

#include <cstring>
#include <map>

namespace {
std::map<const void*, int> g_kind;     // pointers the "GPU" reaches (bit 0) or the CPU shares (bit 1); anything else is pageable
std::map<int, std::vector<char>> g_slot;
int g_queries = 0, g_syncs = 0, g_copies = 0, g_fail_slot = -1, g_checks = 0, g_failed = 0;
void check(bool ok, const char* what) { ++g_checks; if (!ok) { ++g_failed; fprintf(stderr, "FAILED: %s\n", what); } }
}

namespace xsmm {
int pointer_kind(const void* p) { ++g_queries; const auto i = g_kind.find(p); return g_kind.end() != i ? i->second : 0; }
void* scratch(ScratchSlot slot, size_t bytes)
{
  if (slot == g_fail_slot) return nullptr;
  std::vector<char>& v = g_slot[slot];
  if (v.size() < bytes) v.assign(bytes, (char)0x5a); // (exactly as long as asked for: the sanitizer sees a carve that runs over)
  return v.empty() ? nullptr : v.data(); // (as the library's: 0 bytes are answered with what the slot holds, nothing on a fresh thread)
}
int h2d(void* dst, const void* src, size_t bytes) { if (0 == bytes) return 0; ++g_copies; memcpy(dst, src, bytes); return 0; }
int d2h_async(void* dst, const void* src, size_t bytes) { if (0 == bytes) return 0; ++g_copies; memcpy(dst, src, bytes); return 0; }
int copy2d(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t row_bytes, size_t rows, bool)
{
  ++g_copies;
  for (size_t r = 0; r < rows; ++r) memcpy(static_cast<char*>(dst) + r * dst_pitch, static_cast<const char*>(src) + r * src_pitch, row_bytes);
  return 0;
}
int stream_sync() { ++g_syncs; return 0; }
void note_launch(const char*) {}
}

using namespace xsmm;

int main()
{
  { // zero bytes and one byte, pageable: both are staged; a slot with nothing but empty operands asks for no memory (its operand has no
    // device address, and nothing is copied either way); the byte travels both ways, one wait
    char none = 1, one = 7;
    Staged s;
    const Operand* const a = s.out(&none, 0, SLOT_IN0, true);
    const Operand* const b = s.out(&one, 1, SLOT_IN1, true);
    g_copies = 0;
    check(s.place() && nullptr == a->dev && nullptr != a->host && nullptr != b->dev && 7 == *static_cast<char*>(b->dev), "0 and 1 byte: placed and uploaded");
    check(s.back({ a }) && 1 == none, "0 bytes: nothing travels back");
    *static_cast<char*>(b->dev) = 9;
    g_syncs = 0;
    check(s.finish(WAIT_OPERANDS, { b }) && 9 == one && 1 == g_syncs, "1 byte: copied back, one wait");
    check(nullptr == s.in(nullptr, 4, SLOT_IN0) && s.ok(), "no operand: nullptr, still ok");
  }
  { // memory the GPU reaches stays where it is: one query each, no copy; the wait depends on host visibility and on the policy
    char dev[4] = {}, pinned[4] = {};
    g_kind[dev] = 1; g_kind[pinned] = 3;
    Staged s; g_queries = g_copies = g_syncs = 0;
    const Operand* const a = s.in(dev, 4, SLOT_IN0);
    check(s.place() && a->dev == dev && 1 == g_queries && 0 == g_copies, "device operand in place, one query");
    check(s.finish(WAIT_OPERANDS, { a }) && 0 == g_syncs, "device operands: nobody waits");
    Staged t;
    const Operand* const p = t.out(pinned, 4, SLOT_IN1, true);
    check(t.place() && p->dev == pinned && t.finish(WAIT_RESULTS, { p }) && 0 == g_syncs, "host-visible, WAIT_RESULTS: no wait");
    check(t.finish(WAIT_OPERANDS, { p }) && 1 == g_syncs, "host-visible, WAIT_OPERANDS: one wait");
  }
  { // a staged input alone: WAIT_RESULTS does not wait, WAIT_OPERANDS does
    char in[3] = { 1, 2, 3 }, dev[3] = {};
    g_kind[dev] = 1;
    Staged s; g_syncs = 0;
    const Operand* const a = s.in(in, 3, SLOT_IN0);
    const Operand* const r = s.out(dev, 3, SLOT_RESULTS, false);
    check(s.place() && 0 == memcmp(a->dev, in, 3) && s.finish(WAIT_RESULTS, { r }) && 0 == g_syncs, "staged input, device result, WAIT_RESULTS: no wait");
    check(s.finish(WAIT_OPERANDS, { r }) && 1 == g_syncs, "staged input, WAIT_OPERANDS: one wait");
  }
  { // out2d: 3 rows of 5 bytes, 8 apart; the device sees 15 tight bytes, the padding and what follows keep their sentinel
    char host[3 * 8 + 1];
    memset(host, 0x77, sizeof(host));
    for (int r = 0; r < 3; ++r) for (int i = 0; i < 5; ++i) host[r * 8 + i] = (char)(r * 5 + i);
    Staged s;
    const Operand* const c = s.out2d(host, 5, 3, 8, SLOT_C, true);
    check(s.place() && 15 == c->bytes, "out2d placed");
    char* const d = static_cast<char*>(c->dev);
    bool tight = true;
    for (int i = 0; i < 15; ++i) { tight = tight && d[i] == (char)i; d[i] = (char)(100 + i); }
    check(tight, "out2d: tight image uploaded");
    check(s.finish(WAIT_OPERANDS, { c }), "out2d finish");
    bool ok = true;
    for (int r = 0; r < 3; ++r) for (int i = 0; i < 8; ++i) ok = ok && host[r * 8 + i] == (i < 5 ? (char)(100 + r * 5 + i) : (char)0x77);
    check(ok && (char)0x77 == host[24], "out2d: rows back, padding keeps the sentinel");
  }
  { // 24 operands in one slot: carved at 256-byte offsets inside one block, disjoint; the 25th is refused
    char host[STAGED_MAX][3];
    Staged s;
    const Operand* o[STAGED_MAX];
    for (int i = 0; i < STAGED_MAX; ++i) { memset(host[i], i + 1, 3); o[i] = s.out(host[i], 3, SLOT_BLOCK, true); }
    check(s.ok() && s.place(), "24 operands placed");
    bool ok = true;
    for (int i = 0; i < STAGED_MAX; ++i) ok = ok && (size_t)i * 256 == o[i]->offset && (char)(i + 1) == static_cast<char*>(o[i]->dev)[2];
    check(ok && (size_t)STAGED_MAX * 256 == s.total[SLOT_BLOCK], "24 operands: 256-byte carving, each with its bytes");
    for (int i = 0; i < STAGED_MAX; ++i) static_cast<char*>(o[i]->dev)[0] = (char)(50 + i);
    g_syncs = 0;
    check(s.finish(WAIT_OPERANDS, { o[0], nullptr, o[23] }) && 50 == host[0][0] && 73 == host[23][0] && 2 == host[1][0] && 1 == g_syncs, "only the written ones travel back, one wait");
    char more = 0;
    check(nullptr == s.in(&more, 1, SLOT_IN0) && !s.ok() && !s.place(), "the 25th operand is refused");
  }
  { // a failed allocation in the middle: place() says so and uploads nothing behind it
    char a[2] = { 1, 2 }, b[2] = { 3, 4 }, c[2] = { 5, 6 };
    Staged s;
    (void)s.in(a, 2, SLOT_A); (void)s.in(b, 2, SLOT_B); const Operand* const oc = s.out(c, 2, SLOT_C, true);
    g_fail_slot = SLOT_B; g_copies = 0;
    check(!s.place() && !s.ok() && 1 == g_copies && nullptr == oc->dev, "failed allocation in the middle");
    g_fail_slot = -1;
  }
  { // a workspace and staged results in one block
    unsigned result = 0;
    Staged s;
    const Operand* const w = s.work(40, SLOT_HASH);
    const Operand* const r = s.out(&result, sizeof(result), SLOT_HASH, false);
    check(s.place() && static_cast<char*>(r->dev) == static_cast<char*>(w->dev) + 256, "workspace and result share the block");
    *static_cast<unsigned*>(r->dev) = 42u; g_syncs = 0;
    check(s.back({ r }) && 42u == result && 0 == g_syncs && s.copied, "back alone copies and does not wait");
  }
  printf("staging_selftest: %d checks, %d failed\n", g_checks, g_failed);
  return 0 == g_failed ? 0 : 1;
}
