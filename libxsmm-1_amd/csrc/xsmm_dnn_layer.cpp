// xsmm_dnn_layer.cpp -- what the DNN layers share on the host (declared in xsmm_dnn_internal.hpp): layouts, the
// feature-map blocking, the split of a pass over logical threads, the staging of operands in pageable host memory, and the
// report of a failed launch. The templates over the handle type (scratch and tensor binding) are in the header.
#include "xsmm_dnn_internal.hpp"

#include <cstring>

namespace xsmm {

bool layout_dims(libxsmm_dnn_tensor_datalayout* l, unsigned int n, const libxsmm_dnn_tensor_dimtype* types, const unsigned int* sizes)
{
  l->dim_type = static_cast<libxsmm_dnn_tensor_dimtype*>(malloc(n * sizeof(libxsmm_dnn_tensor_dimtype)));
  l->dim_size = static_cast<unsigned int*>(malloc(n * sizeof(unsigned int)));
  if (nullptr == l->dim_type || nullptr == l->dim_size) { free(l->dim_type); free(l->dim_size); l->dim_type = nullptr; l->dim_size = nullptr; return false; }
  l->num_dims = n;
  for (unsigned int i = 0; i < n; ++i) { l->dim_type[i] = types[i]; l->dim_size[i] = sizes[i]; }
  return true;
}

libxsmm_dnn_tensor_datalayout* layout_begin(libxsmm_dnn_err_t* status)
{
  libxsmm_dnn_tensor_datalayout* const l = static_cast<libxsmm_dnn_tensor_datalayout*>(malloc(sizeof(*l)));
  if (nullptr == l) { *status = LIBXSMM_DNN_ERR_CREATE_LAYOUT; return nullptr; }
  memset(l, 0, sizeof(*l));
  return l;
}

libxsmm_dnn_tensor_datalayout* layout_end(libxsmm_dnn_tensor_datalayout* l, bool ok, libxsmm_dnn_err_t* status)
{
  if (!ok) *status = LIBXSMM_DNN_ERR_CREATE_LAYOUT_ARRAYS;
  if (LIBXSMM_DNN_SUCCESS != *status) { free(l->dim_type); free(l->dim_size); free(l); return nullptr; }
  return l;
}

bool is_input(libxsmm_dnn_tensor_type t) { return LIBXSMM_DNN_REGULAR_INPUT == t || LIBXSMM_DNN_GRADIENT_INPUT == t || LIBXSMM_DNN_INPUT == t; }
bool is_output(libxsmm_dnn_tensor_type t) { return LIBXSMM_DNN_REGULAR_OUTPUT == t || LIBXSMM_DNN_GRADIENT_OUTPUT == t || LIBXSMM_DNN_OUTPUT == t; }

FmBlocks feature_map_blocks(int C, bool f32)
{ // libxsmm_dnn_get_feature_map_blocks(C, C) (src/libxsmm_dnn_setup.c:197-252): the output block is 16 whatever C is
  FmBlocks b;
  if (f32) { b.ifmblock = C >= 16 ? 16 : C; b.fm_lp_block = 1; }
  else {
    b.ifmblock = C >= 16 ? 8 : C / 2; b.fm_lp_block = 2;
    if (3 == C) { b.ifmblock = 3; b.fm_lp_block = 1; }
  }
  b.ofmblock = 16;
  b.ifmblock_hp = b.ifmblock * b.fm_lp_block;
  b.ofmblock_lp = b.ofmblock / b.fm_lp_block;
  // (a block of zero divides nothing: the reference would trap; here there are no blocks)
  const int iblock = f32 ? b.ifmblock : b.ifmblock_hp;
  b.blocksifm = 0 < iblock ? C / iblock : 0;
  b.blocksofm = C / b.ofmblock;
  return b;
}

bool activation_layout(libxsmm_dnn_tensor_datalayout* l, libxsmm_dnn_tensor_format format, libxsmm_dnn_datatype datatype_in, libxsmm_dnn_datatype datatype_out,
                       const FmBlocks& b, int N, int C, bool input, unsigned int ifhp, unsigned int ifwp, unsigned int ofhp, unsigned int ofwp, libxsmm_dnn_err_t* status)
{
  typedef libxsmm_dnn_tensor_dimtype D;
  const D dN = LIBXSMM_DNN_TENSOR_DIMTYPE_N, dH = LIBXSMM_DNN_TENSOR_DIMTYPE_H, dW = LIBXSMM_DNN_TENSOR_DIMTYPE_W, dC = LIBXSMM_DNN_TENSOR_DIMTYPE_C;
  const unsigned int n = (unsigned int)N;
  if (0 != (format & LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM)) {
    if (LIBXSMM_DNN_DATATYPE_F32 == datatype_in && LIBXSMM_DNN_DATATYPE_F32 == datatype_out) {
      const D t[5] = { dC, dW, dH, dC, dN };
      const unsigned int in[5] = { (unsigned int)b.ifmblock, ifwp, ifhp, (unsigned int)b.blocksifm, n };
      const unsigned int out[5] = { (unsigned int)b.ofmblock, ofwp, ofhp, (unsigned int)b.blocksofm, n };
      l->datatype = LIBXSMM_DNN_DATATYPE_F32;
      return layout_dims(l, 5, t, input ? in : out);
    }
    const D t[6] = { dC, dC, dW, dH, dC, dN };
    const unsigned int in[6] = { (unsigned int)b.fm_lp_block, (unsigned int)b.ifmblock, ifwp, ifhp, (unsigned int)b.blocksifm, n };
    const unsigned int out[6] = { (unsigned int)b.fm_lp_block, (unsigned int)b.ofmblock_lp, ofwp, ofhp, (unsigned int)b.blocksofm, n };
    l->datatype = LIBXSMM_DNN_DATATYPE_BF16;
    return layout_dims(l, 6, t, input ? in : out);
  }
  if (0 != (format & LIBXSMM_DNN_TENSOR_FORMAT_NHWC)) {
    const D t[4] = { dC, dW, dH, dN };
    const unsigned int in[4] = { (unsigned int)C, ifwp, ifhp, n }, out[4] = { (unsigned int)C, ofwp, ofhp, n };
    l->datatype = datatype_in;
    return layout_dims(l, 4, t, input ? in : out);
  }
  *status = LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  return true;
}

bool thread_share(long long work, int threads, int ltid, long long* b0, long long* b1)
{
  const long long chunk = (0 == work % threads) ? (work / threads) : (work / threads + 1);
  *b0 = (ltid * chunk < work) ? ltid * chunk : work;
  *b1 = ((ltid + 1LL) * chunk < work) ? (ltid + 1LL) * chunk : work;
  return ltid < threads && *b0 < *b1;
}

const Operand* Staging::add(const libxsmm_dnn_tensor* t)
{
  Operand* const o = &op[n++];
  libxsmm_dnn_err_t st;
  o->bytes = (size_t)libxsmm_dnn_get_tensor_elements(t->layout, &st) * libxsmm_dnn_typesize(t->layout->datatype);
  const int kind = pointer_kind(t->data);
  o->dev = t->data; o->host = nullptr; o->offset = 0;
  if (0 != (kind & 2)) wait = true;
  if (0 == (kind & 1)) { o->host = t->data; o->dev = nullptr; o->offset = total; total += (o->bytes + 255) & ~(size_t)255; wait = true; }
  return o;
}

bool Staging::place()
{
  if (0 == total) return true;
  char* const base = static_cast<char*>(scratch(6, total));
  if (nullptr == base) return false;
  for (int i = 0; i < n; ++i) {
    if (nullptr == op[i].host) continue;
    op[i].dev = base + op[i].offset;
    if (0 != h2d(op[i].dev, op[i].host, op[i].bytes)) return false;
  }
  return true;
}

bool Staging::finish(std::initializer_list<const Operand*> written)
{
  for (const Operand* o : written) {
    if (nullptr != o && nullptr != o->host && 0 != d2h(o->host, o->dev, o->bytes)) return false;
  }
  return !wait || 0 == stream_sync();
}

bool launched(const char* name, int hip_error)
{
  note_launch(name);
  if (0 == hip_error) return true;
  fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, hip_error);
  return false;
}

} // namespace xsmm
