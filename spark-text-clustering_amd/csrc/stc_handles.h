// stc_handles.h — the ABI's opaque handles that more than one translation unit fills in (api.hip, text_prep.hip)
#pragma once

#include "stc_internal.h"

struct stc_ctx : stc::Ctx {};
struct stc_dtok {
  stc::Ctx* ctx = nullptr;  // the context it was uploaded on / made by; only it may read the buffers
  int device = -1;          // for stc_tokens_free, which may run after that context is gone
  stc::DevBuf utf8, tok_off, doc_off;
  int64_t n_bytes = 0, n_tok = 0, n_docs = 0;
  int64_t max_doc = -1;  // the longest document's token count (from the upload's offsets)
  bool off32 = false;    // tok_off holds u32 offsets (blob + padding < 4 GiB), else int64
};
