// fid_gallery, for the translation units that own parts of it: match.hip (the fp16 rows) and coarse.hip (their int8 copy).
#pragma once
#include "common.h"

struct fid_gallery {
    int G = 0, Gp = 0, dim = 0;
    void *unit_f16 = nullptr;  // [Gp][dim], rows >= G are zero
    // the quantised copy of the coarse search (quant_core.h): allocated by fid_gallery_quantize only, NULL in a gallery that never asked for it
    int8_t *codes_i8 = nullptr;  // [Gp][dim]
    int8_t *exps_i8 = nullptr;   // [Gp]
};

namespace fid {
// requantise gallery rows rows_dev[0 .. n) from unit_f16 (entries outside [0, G) are skipped); the quantised copy exists, the mutex is held
void requantize_rows(fid_ctx *ctx, fid_gallery *g, const int *rows_dev, int n);
}  // namespace fid
