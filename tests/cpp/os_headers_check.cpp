// Check of the host column-header parse (noetic-slam_amd/csrc/os_headers.h) on the CPU:
//   * with arguments `profile h columns_per_packet w packets.bin out.bin`: the headers of the
//     packets in packets.bin (back to back) are written to out.bin as timestamp (u64 x w),
//     status (u32 x w), measurement_id (u16 x w), for the caller to compare;
//   * always: random-byte packets of all four profiles at several sizes, in heap buffers of the
//     exact size (a read past a packet shows under AddressSanitizer), against a restatement that
//     walks the columns with its own offsets; the argument rules (NULL pointers, bad formats,
//     zero packets).
// Exits non-zero on the first miss.  Built plain and with -fsanitize=address,undefined
// (tests/test_deskew_headers.py).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../noetic-slam_amd/csrc/os_headers.h"

using namespace tsdf;

static int fails = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            if (++fails > 10) return;     \
        }                                 \
    } while (0)

static uint64_t rd(const std::vector<uint8_t>& b, size_t at, int n) {
    uint64_t v = 0;
    for (int k = n - 1; k >= 0; k--) v = v * 256 + b.at(at + k);
    return v;
}

static void random_packets() {
    std::mt19937_64 rng(20241);
    const uint32_t pixel_bytes[4] = {12, 12, 16, 4};
    for (uint32_t profile = 0; profile < 4; profile++)
        for (uint32_t h : {1u, 8u, 33u, 128u})
            for (uint32_t cpp : {1u, 16u})
                for (uint32_t n_packets : {0u, 1u, 5u}) {
                    const uint32_t w = 64;
                    const tsdf_os_format fmt = {profile, h, cpp, w};
                    const bool legacy = profile == 0;
                    const size_t col = (legacy ? 16 : 12) + (size_t)h * pixel_bytes[profile] +
                                       (legacy ? 4 : 0);
                    const size_t pkt = (legacy ? 0 : 64) + cpp * col;
                    std::vector<uint8_t> buf(pkt * n_packets);
                    for (auto& x : buf) x = (uint8_t)rng();
                    // keep some ids in range: random 16-bit ids are mostly >= w
                    for (size_t c = 0; c < (size_t)n_packets * cpp; c += 2) {
                        const size_t at = (c / cpp) * pkt + (legacy ? 0 : 32) + (c % cpp) * col;
                        buf[at + 8] = (uint8_t)(rng() % (w + 4));
                        buf[at + 9] = 0;
                    }
                    std::vector<uint64_t> ts(w, 7), ets(w, 0);
                    std::vector<uint32_t> st(w, 7), est(w, 0);
                    std::vector<uint16_t> mid(w, 7), emid(w, 0);
                    const int rc = os_headers(&fmt, buf.data(), n_packets, ts.data(), st.data(),
                                              mid.data());
                    CHECK(rc == TSDF_OK, "rc %d", rc);
                    for (uint32_t p = 0; p < n_packets; p++)
                        for (uint32_t c = 0; c < cpp; c++) {
                            const size_t at = p * pkt + (legacy ? 0 : 32) + c * col;
                            const uint64_t m = rd(buf, at + 8, 2);
                            const uint64_t s = legacy ? rd(buf, at + col - 4, 4) : rd(buf, at + 10, 2);
                            if (m >= w || s % 2 == 0) continue;
                            ets[m] = rd(buf, at, 8);
                            est[m] = (uint32_t)s;
                            emid[m] = (uint16_t)m;
                        }
                    CHECK(ts == ets && st == est && mid == emid, "profile %u h %u cpp %u n %u",
                          profile, h, cpp, n_packets);
                }
}

static void arguments() {
    const tsdf_os_format fmt = {1, 8, 16, 64};
    uint64_t ts[64];
    uint32_t st[64];
    uint16_t mid[64];
    uint8_t one = 0;
    CHECK(os_headers(&fmt, nullptr, 0, ts, st, mid) == TSDF_OK, "zero packets");
    CHECK(os_headers(&fmt, nullptr, 1, ts, st, mid) == TSDF_EINVAL, "null packets");
    CHECK(os_headers(nullptr, &one, 0, ts, st, mid) == TSDF_EINVAL, "null format");
    CHECK(os_headers(&fmt, &one, 0, nullptr, st, mid) == TSDF_EINVAL, "null timestamp");
    CHECK(os_headers(&fmt, &one, 0, ts, nullptr, mid) == TSDF_EINVAL, "null status");
    CHECK(os_headers(&fmt, &one, 0, ts, st, nullptr) == TSDF_EINVAL, "null measurement_id");
    for (const tsdf_os_format bad : {tsdf_os_format{4, 8, 16, 64}, tsdf_os_format{1, 0, 16, 64},
                                     tsdf_os_format{1, 8, 0, 64}, tsdf_os_format{1, 8, 16, 0},
                                     tsdf_os_format{1, 4097, 16, 64}})
        CHECK(os_headers(&bad, &one, 0, ts, st, mid) == TSDF_EINVAL, "bad format");
}

static int from_file(char** a) {
    const tsdf_os_format fmt = {(uint32_t)std::atoi(a[1]), (uint32_t)std::atoi(a[2]),
                                (uint32_t)std::atoi(a[3]), (uint32_t)std::atoi(a[4])};
    OsLayout L;
    if (!os_layout(&fmt, L)) return 2;
    std::FILE* f = std::fopen(a[5], "rb");
    if (!f) return 2;
    std::vector<uint8_t> buf;
    uint8_t chunk[4096];
    for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;)
        buf.insert(buf.end(), chunk, chunk + n);
    std::fclose(f);
    if (buf.size() % L.packet_bytes) return 2;
    std::vector<uint64_t> ts(fmt.columns_per_frame);
    std::vector<uint32_t> st(fmt.columns_per_frame);
    std::vector<uint16_t> mid(fmt.columns_per_frame);
    if (os_headers(&fmt, buf.data(), (uint32_t)(buf.size() / L.packet_bytes), ts.data(), st.data(),
                   mid.data()) != TSDF_OK)
        return 2;
    std::FILE* o = std::fopen(a[6], "wb");
    if (!o) return 2;
    std::fwrite(ts.data(), 8, ts.size(), o);
    std::fwrite(st.data(), 4, st.size(), o);
    std::fwrite(mid.data(), 2, mid.size(), o);
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7 && from_file(argv)) {
        std::printf("cannot parse the packets file\n");
        return 1;
    }
    random_packets();
    arguments();
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
