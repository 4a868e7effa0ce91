// The crop stage's arithmetic (csrc/crop_math.h) on the host, for tests/test_crop_math_host.py: the functions the kernels
// call, run over plain buffers in the multi-pass form (plan -> horizontal pass -> vertical pass -> INTER_AREA), so that the
// oracle pins them without a GPU. Built with the host C++ compiler alone, -ffp-contract=off like the kernels.
//
//   crop_math_table IN OUT      IN starts with an int32 mode; all integers little-endian int32, boxes float64
//
// mode 1, square crops:  n_frames H W n_cases out_size | frames u8[n_frames][H][W][3] | per case: frame padding box[4]
//         -> status[n_cases] (as the library reports it) | crops u8[n_cases][S][S][3] (failed crops all zero)
// mode 2, images:        n swap_rb | per image: h w out_w | the images u8[h][w][3], concatenated
//         out_w == 0: the runner's input branch -> u8[128][128][3]; out_w > 0: imutils.resize(width = out_w) of the
//         rectangle -> u8[int(h * (out_w / float(w)))][out_w][3]
//         -> status[n] | the outputs, concatenated
// mode 3, digit form:    n_pairs | per pass: in_size out_size
//         -> n_rows n_coef | per output coordinate: taps constant | per tap the row holds (at most 15), every coordinate in
//            turn: k d0 d1 d2
#include "../../playaid_core_amd/csrc/crop_math.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pa;

namespace {

struct Reader {
    std::vector<uint8_t> buf;
    size_t at = 0;
    const uint8_t* take(size_t n) {
        if (n > buf.size() - at) {
            fprintf(stderr, "crop_math_table: input ends early\n");
            exit(2);
        }
        const uint8_t* p = buf.data() + at;
        at += n;
        return p;
    }
    int32_t i32() {
        int32_t v;
        memcpy(&v, take(4), 4);
        return v;
    }
    double f64() {
        double v;
        memcpy(&v, take(8), 8);
        return v;
    }
};

void put(FILE* f, const void* p, size_t n) {
    if (n && fwrite(p, 1, n, f) != n) {
        fprintf(stderr, "crop_math_table: write failed\n");
        exit(2);
    }
}

std::vector<int32_t> table(int in_size, int out_size) {
    std::vector<int32_t> t((size_t)out_size * COEF_ROW);
    bicubic_coef_table(in_size, out_size, t.data(), 0, 1);
    return t;
}

void square_crops(Reader& in, FILE* out) {
    const int n_frames = in.i32(), H = in.i32(), W = in.i32(), n = in.i32(), S = in.i32();
    const uint8_t* frames = in.take((size_t)n_frames * H * W * 3);
    std::vector<int32_t> status(n);
    std::vector<uint8_t> crops((size_t)n * S * S * 3, 0);
    for (int i = 0; i < n; ++i) {
        const int frame = in.i32(), pad = in.i32();
        double box[4];
        for (double& v : box) v = in.f64();
        const CropPlan pl = square_crop_plan(box, W, H, pad, S, SIZE_MAX, INT_MAX, frame, (unsigned)frame < (unsigned)n_frames);
        status[i] = pl.status == PA_CROP_BLANK ? PA_CROP_OK : pl.status;
        if (pl.status != PA_CROP_OK) continue;
        Canvas cv;
        cv.px = pl.px; cv.py = pl.py; cv.rw = pl.rw; cv.rh = pl.rh;
        cv.src = frames + (((size_t)pl.frame * H + pl.sy0) * W + pl.sx0) * 3;
        cv.pitch = (size_t)W * 3;
        std::vector<uint8_t> t1, t2;
        if (pl.need_h) {
            t1.resize((size_t)pl.sh * pl.rw * 3);
            bicubic_pass_h(table(pl.sw, pl.rw).data(), cv.src, cv.pitch, pl.sh, pl.rw, t1.data(), 0, 1);
            cv.src = t1.data();
            cv.pitch = (size_t)pl.rw * 3;
        }
        if (pl.need_v) {
            t2.resize((size_t)pl.rh * pl.rw * 3);
            bicubic_pass_v(table(pl.sh, pl.rh).data(), cv.src, cv.pitch, pl.rh, pl.rw, t2.data(), 0, 1);
            cv.src = t2.data();
            cv.pitch = (size_t)pl.rw * 3;
        }
        const AreaGeom g = area_geom(pl, S);
        uint8_t* o = crops.data() + (size_t)i * S * S * 3;
        for (int dy = 0; dy < pl.out_h; ++dy)
            for (int dx = 0; dx < S; ++dx, o += 3) {
                int o0, o1, o2;
                area_pixel(g, cv, dy, dx, o0, o1, o2);
                o[0] = (uint8_t)o0; o[1] = (uint8_t)o1; o[2] = (uint8_t)o2;
            }
    }
    put(out, status.data(), status.size() * 4);
    put(out, crops.data(), crops.size());
}

void resize_area(const AreaGeom g, const uint8_t* img, std::vector<uint8_t>& dst) {
    WhCanvas cv;
    cv.src = img;
    cv.pitch = g.sw * 3;
    dst.assign((size_t)g.oh * g.ow * 3, 0);
    uint8_t* o = dst.data();
    for (int dy = 0; dy < g.oh; ++dy)
        for (int dx = 0; dx < g.ow; ++dx, o += 3) {
            int o0, o1, o2;
            area_pixel(g, cv, dy, dx, o0, o1, o2);
            o[0] = (uint8_t)o0; o[1] = (uint8_t)o1; o[2] = (uint8_t)o2;
        }
}

void images(Reader& in, FILE* out) {
    const int n = in.i32(), swap_rb = in.i32();
    std::vector<int32_t> hs(n), ws(n), ows(n), status(n);
    for (int i = 0; i < n; ++i) {
        hs[i] = in.i32();
        ws[i] = in.i32();
        ows[i] = in.i32();
    }
    std::vector<uint8_t> all;
    for (int i = 0; i < n; ++i) {
        const int h = hs[i], w = ws[i];
        const uint8_t* img = in.take((size_t)h * w * 3);
        std::vector<uint8_t> res, a, b;
        if (ows[i] > 0) {  // a rectangle: imutils.resize(width = out_w)
            const int oh = (int)((double)h * ((double)ows[i] / (double)w));
            status[i] = oh < 1 ? PA_CROP_EMPTY : PA_CROP_OK;
            if (oh >= 1) resize_area(area_branch(w, h, ows[i], oh), img, res);
        } else {
            const RunnerInPlan pl = runner_in_plan(w, h, SIZE_MAX);
            status[i] = pl.status;
            res.assign((size_t)PA_CROP * PA_CROP * 3, 0);
            if (pl.status == PA_CROP_OK) {
                resize_area(pl.area, img, a);
                const uint8_t* cur = a.data();
                if (pl.need_h) {
                    b.resize((size_t)pl.area.oh * pl.rw * 3);
                    bicubic_pass_h(table(PA_CROP, pl.rw).data(), a.data(), (size_t)PA_CROP * 3, pl.area.oh, pl.rw, b.data(), 0, 1);
                    cur = b.data();
                }
                std::vector<int32_t> cv;
                if (pl.need_v) cv = table(pl.area.oh, pl.rh);
                for (int p = 0; p < PA_CROP * PA_CROP; ++p) {
                    int o0, o1, o2;
                    runner_in_pixel(pl, cur, cv.data(), p, o0, o1, o2);
                    res[(size_t)p * 3 + 0] = (uint8_t)(swap_rb ? o2 : o0);
                    res[(size_t)p * 3 + 1] = (uint8_t)o1;
                    res[(size_t)p * 3 + 2] = (uint8_t)(swap_rb ? o0 : o2);
                }
            }
        }
        all.insert(all.end(), res.begin(), res.end());
    }
    put(out, status.data(), status.size() * 4);
    put(out, all.data(), all.size());
}

void digits(Reader& in, FILE* out) {
    const int n_pairs = in.i32();
    std::vector<int32_t> rows, coefs;
    for (int i = 0; i < n_pairs; ++i) {
        const int in_size = in.i32(), out_size = in.i32();
        const std::vector<int32_t> t = table(in_size, out_size);
        for (int xx = 0; xx < out_size; ++xx) {
            const int32_t* row = t.data() + (size_t)xx * COEF_ROW;
            rows.push_back(row[1]);
            rows.push_back(coef_row_constant(row));
            for (int k = 0; k < row[1] && k < PA_KSIZE_MAX; ++k) {  // (a wider pass is refused; the row holds its first taps)
                int d0, d1, d2;
                coef_digits(row[2 + k], &d0, &d1, &d2);
                coefs.insert(coefs.end(), {row[2 + k], d0, d1, d2});
            }
        }
    }
    const int32_t head[2] = {(int32_t)(rows.size() / 2), (int32_t)(coefs.size() / 4)};
    put(out, head, sizeof head);
    put(out, rows.data(), rows.size() * 4);
    put(out, coefs.data(), coefs.size() * 4);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: crop_math_table IN OUT\n");
        return 2;
    }
    Reader in;
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    fseek(f, 0, SEEK_END);
    in.buf.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(in.buf.data(), 1, in.buf.size(), f) != in.buf.size()) return 2;
    fclose(f);
    FILE* out = fopen(argv[2], "wb");
    if (!out) {
        perror(argv[2]);
        return 2;
    }
    const int mode = in.i32();
    if (mode == 1) square_crops(in, out);
    else if (mode == 2) images(in, out);
    else if (mode == 3) digits(in, out);
    else return 2;
    return fclose(out) == 0 ? 0 : 2;
}
