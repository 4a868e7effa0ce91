// The pa_encoder handle (pa_encoder_create, transformer.hip), shared with its trainer (encoder_train.hip), which borrows the
// weights.
#pragma once
#include "pa_kernels.h"
#include <cstdint>
#include <string>
#include <vector>

struct pa_encoder {
    int in_dim = 0, hidden = 0, slots = 0, enc_dim = 0, heads = 0, layers = 0, ff = 0, actions = 0, max_rows = 0, D = 0, device = 0;
    float* weights = nullptr;
    float *ffn_w = nullptr, *ffn_b = nullptr, *enc = nullptr, *cls_w = nullptr, *cls_b = nullptr;
    float* ffn_pad = nullptr;  // [D][in_dim] + [D]: the front projection with zero rows for the encoding's columns, so that its
                               // N is whole matrix tiles (247 -> 256) and it runs on the MFMA kernel; append_encoding overwrites them
    struct Layer { float *in_w, *in_b, *out_w, *out_b, *l1_w, *l1_b, *l2_w, *l2_b, *n1_g, *n1_b, *n2_g, *n2_b; };
    std::vector<Layer> layer;
    float *x = nullptr, *qkv = nullptr, *att = nullptr, *y = nullptr, *f1 = nullptr;
    std::string last_error;
};

namespace pa {

// floats of the blob behind its header: resnet_ffn weight and bias, the time encoding, per layer in_proj, out_proj, linear1,
// linear2 (weight, bias each), norm1, norm2 (weight, bias each), then the classifier (PyTorch layouts)
inline size_t encoder_float_count(int in_dim, int hidden, int slots, int enc_dim, int layers, int ff, int actions) {
    const size_t D = (size_t)hidden + enc_dim;
    size_t n = (size_t)hidden * in_dim + hidden + (size_t)slots * enc_dim;
    n += (size_t)layers * (3 * D * D + 3 * D + D * D + D + (size_t)ff * D + ff + D * ff + D + 4 * D);
    n += (size_t)actions * D + actions;
    return n;
}

}  // namespace pa
