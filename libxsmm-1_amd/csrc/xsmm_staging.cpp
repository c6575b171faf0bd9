// xsmm_staging.cpp -- operands in any memory for every entry point that takes them (Staged, declared in xsmm_internal.hpp;
// DESIGN.md 8w), and the one report of a kernel launch. Host code on top of pointer_kind, scratch, h2d, d2h_async, copy2d and
// stream_sync alone: tools/staging_selftest.cpp drives it against stand-ins for those.
#include "xsmm_internal.hpp"

namespace xsmm {

Operand* Staged::carve(size_t bytes, ScratchSlot slot)
{
  if (STAGED_MAX <= n) { failed = true; return nullptr; }
  Operand* const o = &op[n++];
  o->dev = nullptr; o->host = nullptr; o->bytes = bytes; o->slot = slot; o->upload = false; o->row_bytes = o->pitch = 0;
  o->offset = total[slot]; total[slot] += (bytes + 255) & ~(size_t)255;
  return o;
}

const Operand* Staged::add(void* p, size_t bytes, ScratchSlot slot, bool upload, size_t row_bytes, size_t pitch)
{
  if (nullptr == p) return nullptr;
  const int kind = pointer_kind(p);
  if (0 != (kind & 2)) visible = true;
  Operand* o;
  if (0 == (kind & 1)) {
    o = carve(bytes, slot);
    if (nullptr == o) return nullptr;
    o->host = p; o->upload = upload; o->row_bytes = row_bytes; o->pitch = pitch;
    staged = true;
  }
  else {
    if (STAGED_MAX <= n) { failed = true; return nullptr; }
    o = &op[n++];
    o->dev = p; o->host = nullptr; o->bytes = bytes; o->offset = 0; o->slot = -1; o->upload = false; o->row_bytes = o->pitch = 0;
  }
  return o;
}

const Operand* Staged::work(size_t bytes, ScratchSlot slot) { return carve(bytes, slot); }

bool Staged::place()
{
  if (failed) return false;
  char* base[SLOT_COUNT] = {};
  for (int i = 0; i < n; ++i) { // (the first operand of a slot allocates the block of all of them)
    Operand& o = op[i];
    if (0 > o.slot) continue;
    if (0 == total[o.slot]) continue; // (nothing but empty operands: no memory is asked for, dev stays nullptr)
    if (nullptr == base[o.slot]) base[o.slot] = static_cast<char*>(scratch((ScratchSlot)o.slot, total[o.slot]));
    if (nullptr == base[o.slot]) { failed = true; return false; }
    o.dev = base[o.slot] + o.offset;
    if (!o.upload) continue;
    const int e = (0 == o.pitch) ? h2d(o.dev, o.host, o.bytes)
      : (0 != o.bytes ? copy2d(o.dev, o.row_bytes, o.host, o.pitch, o.row_bytes, o.bytes / o.row_bytes, true) : 0);
    if (0 != e) { failed = true; return false; }
  }
  return true;
}

bool Staged::back(std::initializer_list<const Operand*> written)
{
  for (const Operand* o : written) {
    if (nullptr == o || nullptr == o->host) continue;
    const int e = (0 == o->pitch) ? d2h_async(o->host, o->dev, o->bytes)
      : (0 != o->bytes ? copy2d(o->host, o->pitch, o->dev, o->row_bytes, o->row_bytes, o->bytes / o->row_bytes, false) : 0);
    if (0 != e) return false;
    copied = true;
  }
  return true;
}

bool Staged::finish(WaitFor wait, std::initializer_list<const Operand*> written)
{
  if (!back(written)) return false;
  return !(copied || (WAIT_OPERANDS == wait && (staged || visible))) || 0 == stream_sync();
}

namespace {
bool report(const char* name, int hip_error, bool count_failed)
{
  if (0 == hip_error || count_failed) note_launch(name);
  if (0 == hip_error) return true;
  fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, hip_error);
  return false;
}
}

bool launched(const char* name, int hip_error) { return report(name, hip_error, true); }
bool queued(const char* name, int hip_error) { return report(name, hip_error, false); }

} // namespace xsmm
