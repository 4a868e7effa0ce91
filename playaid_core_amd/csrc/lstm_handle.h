// The pa_lstm handle (pa_lstm_create, lstm.hip), shared with its trainer (lstm_train.hip), which borrows the weights.
#pragma once
#include "pa_kernels.h"
#include <cstdint>
#include <string>
#include <vector>

struct pa_lstm {
    int in_dim = 0, hid = 0, layers = 0, actions = 0, max_rows = 0, device = 0;
    std::vector<float*> w_ih, w_hh, b_ih, b_hh;
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
    float *weights = nullptr;            // one allocation behind all of the above
    float *pre = nullptr, *hseq[2] = {nullptr, nullptr}, *c = nullptr;
    int* sync_words = nullptr;            // [2 * layers]: per layer an unused word and the error word of its launch
    unsigned long long* gran = nullptr;   // [2][LSTM_NMAX][512] h granules {value, tag} of the layer in flight
    unsigned long long* dbg = nullptr;    // PA_LSTM_STAMP=1: in-kernel clock sums of the last layer launch
    int* sync_host = nullptr;             // pinned copy of the error words
    hipEvent_t sync_ev = nullptr;         // behind the last forward's copies into sync_host: the host reads the words only once it is done
    bool sync_pending = false;            // a forward has been enqueued since the words were last read
    int occ_blocks = -1, occ_key = -1;    // co-resident lstm_layer_kernel workgroups the device holds for batch * 16 + U == occ_key
    bool persistent = true;               // one launch per layer (lstm_layer_kernel); false after a barrier timeout
    std::vector<int32_t> forms;           // per layer: the pa_lstm_form the last forward launched it as (pa_lstm_layer_forms)
    std::string last_error;
};

namespace pa {

// floats of the blob behind its header: per layer w_ih, w_hh, b_ih, b_hh, then the decoder's w1, b1, w2, b2 (PyTorch layouts)
inline size_t lstm_float_count(int in_dim, int hid, int layers, int actions) {
    size_t n = 0;
    for (int l = 0; l < layers; ++l) n += (size_t)4 * hid * (l == 0 ? in_dim : hid) + (size_t)4 * hid * hid + 8 * (size_t)hid;
    n += (size_t)128 * hid + 128 + (size_t)actions * 128 + actions;
    return n;
}

}  // namespace pa
