// A stand-alone program over the host half of the JPEG reader's piece-wise entropy stage (csrc/jpeg_sync.hpp, csrc/jpeg_entropy.hpp),
// built by tests/test_jpeg_sync_sanitizer.py with -fsanitize=address,undefined: plain C++, no GPU runtime, no library of the project.
//
//     jpeg_sync_sanitize FILE...
//
// Every truncation and every single-bit flip of every FILE goes, in a heap block of exactly its size, through the header walk, the
// segment table and jpeg_sync_entropy_host at pieces of 16 and 128 bytes, and through the serial walk beside it: the flags must
// agree, and the coefficients where the flag is 0. The sanitizers end the process at a read or a write outside a block, at a signed
// overflow, a shift or an index out of range; a disagreement ends it with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define DAD3D_HD inline
#include "../dad-3dheads_amd/csrc/jpeg_sync.hpp"

using namespace dad3d;

static long long tried = 0, flagged = 0, in_pieces = 0, serially = 0;

static bool one(const std::vector<unsigned char>& bytes) {
    const long long size = (long long)bytes.size();
    unsigned char* file = static_cast<unsigned char*>(std::malloc(size ? size : 1));  // exactly the file: a byte beyond it is a finding
    if (size) std::memcpy(file, bytes.data(), size);
    JpegFile* F = new JpegFile();
    bool ok = true;
    int flag = jpeg_parse_header(file, size, *F);
    if (!flag) {
        const long long blocks = jpeg_block_capacity(F->h, F->w, F->comps);
        long long cap = jpeg_segment_capacity(F->h, F->w, size);
        cap = cap < 1 ? 1 : cap;
        JpegSegment* segs = new JpegSegment[cap];
        flag = jpeg_find_segments(file, size, *F, segs, cap);
        if (!flag) {
            short* serial = new short[(size_t)blocks * 64];
            int serial_flag = 0;
            for (int seg = 0; !serial_flag && seg < F->nseg; ++seg) serial_flag = jpeg_decode_segment(file, *F, seg, segs[seg], serial);
            const int total = jpeg_total_blocks(*F);
            for (int piece_bytes = 16; piece_bytes <= 128; piece_bytes *= 8) {
                short* coefs = new short[(size_t)blocks * 64];
                int info[4];
                const int got = jpeg_sync_entropy_host(file, *F, segs, piece_bytes, coefs, info);
                if (got != serial_flag || (!got && std::memcmp(coefs, serial, (size_t)total * 128) != 0)) {
                    std::fprintf(stderr, "a file of %lld bytes at pieces of %d: flag %d, serially %d, or other coefficients\n", size, piece_bytes, got,
                                 serial_flag);
                    ok = false;
                }
                in_pieces += info[0] == 1, serially += info[0] == 2;
                delete[] coefs;
            }
            flag = serial_flag;
            delete[] serial;
        }
        delete[] segs;
    }
    ++tried, flagged += flag != 0;
    delete F;
    std::free(file);
    return ok;
}

int main(int argc, char** argv) {
    bool ok = argc > 1;
    for (int a = 1; a < argc; ++a) {
        std::FILE* in = std::fopen(argv[a], "rb");
        if (!in) {
            std::fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<unsigned char> whole;
        unsigned char chunk[4096];
        for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, in)) > 0;) whole.insert(whole.end(), chunk, chunk + n);
        std::fclose(in);
        ok = one(whole) && ok;
        for (size_t n = 0; n < whole.size(); ++n) ok = one(std::vector<unsigned char>(whole.begin(), whole.begin() + n)) && ok;
        for (size_t at = 0; at < whole.size(); ++at)
            for (int bit = 0; bit < 8; ++bit) {
                std::vector<unsigned char> flipped(whole);
                flipped[at] ^= (unsigned char)(1u << bit);
                ok = one(flipped) && ok;
            }
    }
    std::printf("%lld files, %lld flagged, %lld walks in pieces, %lld serial because not verified\n", tried, flagged, in_pieces, serially);
    return ok ? 0 : 1;
}
