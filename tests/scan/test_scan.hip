// test_scan -- the scan primitives of queryengine_amd/csrc/qe_scan.h, called directly through libqe_hip.so and compared
// with host loops.  Everything is an integer, so every comparison is exact.  Exit status 0 and one "passed" line, or 1 with
// the first mismatch printed; 2 when there is no GPU (no CPU fallback).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../queryengine_amd/csrc/qe_scan.h"

using namespace qe;

namespace {

int g_checks = 0;

#define HIP_OK(e)                                                                                 \
    do {                                                                                          \
        const hipError_t err_ = (e);                                                              \
        if (err_ != hipSuccess) {                                                                 \
            std::printf("HIP error %s at %s:%d\n", hipGetErrorString(err_), __FILE__, __LINE__);  \
            std::exit(3);                                                                         \
        }                                                                                         \
    } while (0)

[[noreturn]] void mismatch(const std::string &what, long long at, unsigned long long got, unsigned long long want) {
    std::printf("MISMATCH %s at %lld: got %llu, want %llu\n", what.c_str(), at, got, want);
    std::exit(1);
}

struct Lcg {
    u64 s;
    u32 next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (u32)(s >> 33);
    }
};

// a device copy of a host vector, read back into it by fetch()
template <typename T> struct Dev {
    T *p = nullptr;
    size_t n;
    explicit Dev(const std::vector<T> &h) : n(h.size()) {
        HIP_OK(hipMalloc(&p, (n ? n : 1) * sizeof(T)));
        if (n) HIP_OK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
    }
    ~Dev() { (void)hipFree(p); }
    std::vector<T> fetch() const {
        std::vector<T> h(n);
        if (n) HIP_OK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
};

template <typename T> void expect_equal(const std::string &what, const std::vector<T> &got, const std::vector<T> &want) {
    for (size_t i = 0; i < want.size(); i++)
        if (got[i] != want[i]) mismatch(what, (long long)i, (u64)got[i], (u64)want[i]);
    g_checks++;
}

constexpr int kGuard = 8;   // elements behind every output that must keep their fill

// ---- launch_carry_scan -----------------------------------------------------------------------------------------------------
template <typename T, int THREADS> void carry_case(int64_t n, int nlists, u64 scale, bool with_totals) {
    const std::string what = "carry_scan<" + std::to_string(sizeof(T) * 8) + " bit, " + std::to_string(THREADS) + "> n=" + std::to_string(n) +
                             " lists=" + std::to_string(nlists) + (scale > 1 ? " wide" : "") + (with_totals ? "" : " no totals");
    Lcg r{(u64)n * 977 + (u64)nlists};
    std::vector<T> a((size_t)(n * nlists) + kGuard);
    for (size_t i = 0; i < a.size(); i++) a[i] = (T)((u64)(r.next() % 1000u) * scale);
    std::vector<T> want = a;
    std::vector<u64> want_tot((size_t)nlists + kGuard, 0xA5A5A5A5A5A5A5A5ull);
    for (int l = 0; l < nlists; l++) {
        u64 sum = 0;
        for (int64_t i = 0; i < n; i++) {
            want[(size_t)(i * nlists + l)] = (T)sum;
            sum += (u64)a[(size_t)(i * nlists + l)];
        }
        want_tot[(size_t)l] = sum;
    }
    Dev<T> d(a);
    Dev<u64> tot(std::vector<u64>((size_t)nlists + kGuard, 0xA5A5A5A5A5A5A5A5ull));
    launch_carry_scan<T, THREADS>(nullptr, d.p, n, nlists, with_totals ? tot.p : nullptr);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    expect_equal(what, d.fetch(), want);
    if (!with_totals) want_tot.assign(want_tot.size(), 0xA5A5A5A5A5A5A5A5ull);
    expect_equal(what + " totals", tot.fetch(), want_tot);
}

template <typename T, int THREADS> void carry_cases() {
    const int64_t ns[] = {0, 1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, 3 * THREADS + 7};
    for (int64_t n : ns)
        for (int nlists : {1, 3}) carry_case<T, THREADS>(n, nlists, 1, true);
}

// ---- exclusive_scan ------------------------------------------------------------------------------------------------------
template <typename T> void exclusive_case(int64_t n, bool in_place) {
    const std::string what = "exclusive_scan<" + std::to_string(sizeof(T) * 8) + " bit> n=" + std::to_string(n) + (in_place ? " in place" : "");
    Lcg r{(u64)n * 31 + 7};
    std::vector<T> in((size_t)n + kGuard);
    for (size_t i = 0; i < in.size(); i++) in[i] = (T)(r.next() & 3u);
    std::vector<T> want((size_t)n + kGuard, (T)0x5A5A5A5A);
    if (in_place) want = in;
    u64 sum = 0;
    for (int64_t i = 0; i < n; i++) {
        want[(size_t)i] = (T)sum;
        sum += (u64)in[(size_t)i];
    }
    Dev<T> d_in(in), d_out(std::vector<T>((size_t)n + kGuard, (T)0x5A5A5A5A)), sums(std::vector<T>((size_t)scan_blocks(n)));
    Dev<u64> tot(std::vector<u64>(1, 0));
    exclusive_scan<T>(nullptr, ArrayLoad<T>{d_in.p}, in_place ? d_in.p : d_out.p, sums.p, n, tot.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    expect_equal(what, in_place ? d_in.fetch() : d_out.fetch(), want);
    if (!in_place) expect_equal(what + " input untouched", d_in.fetch(), in);
    expect_equal(what + " total", tot.fetch(), std::vector<u64>(1, sum));
}

// ---- bitmap_ranks + bitmap_positions -----------------------------------------------------------------------------------------
constexpr u32 kFill = 0xA5A5A5A5u;

// v (and k, if not empty) are whole words whose bits past n are set on purpose: they must not count
void bitmap_case(const std::string &name, int64_t n, std::vector<u64> v, std::vector<u64> k) {
    const int64_t nw = (n + 63) / 64;
    if (n & 63) {
        v[(size_t)nw - 1] |= ~0ull << (n & 63);
        if (!k.empty()) k[(size_t)nw - 1] |= ~0ull << (n & 63);
    }
    const std::string what = "bitmap " + name + " n=" + std::to_string(n) + (k.empty() ? "" : " masked");
    std::vector<u32> want_prefix((size_t)nw + 1 + kGuard, kFill), want_pos;
    for (int64_t i = 0; i < n; i++) {
        if ((i & 63) == 0) want_prefix[(size_t)(i >> 6)] = (u32)want_pos.size();
        const u64 w = v[(size_t)(i >> 6)] & (k.empty() ? ~0ull : k[(size_t)(i >> 6)]);
        if ((w >> (i & 63)) & 1ull) want_pos.push_back((u32)i);
    }
    const int64_t total = (int64_t)want_pos.size();
    want_prefix[(size_t)nw] = (u32)total;

    Dev<u64> dv(v), dk(k), tot(std::vector<u64>(1, 0));
    const u64 *kp = k.empty() ? nullptr : dk.p;
    Dev<u32> prefix(std::vector<u32>((size_t)nw + 1 + kGuard, kFill)), sums(std::vector<u32>((size_t)scan_blocks(nw + 1)));
    bitmap_ranks(nullptr, (const uint64_t *)dv.p, (const uint64_t *)kp, n, prefix.p, sums.p, tot.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    expect_equal(what + " prefix", prefix.fetch(), want_prefix);
    expect_equal(what + " total", tot.fetch(), std::vector<u64>(1, (u64)total));

    // with the sentinel and room for exactly total + 1 entries; then with less room than there are positions
    for (const int64_t capacity : {total + 1, total / 2}) {
        std::vector<u32> want((size_t)total + 1 + kGuard, kFill);
        for (int64_t j = 0; j < total && j < capacity; j++) want[(size_t)j] = want_pos[(size_t)j];
        if (total < capacity) want[(size_t)total] = (u32)n;
        Dev<u32> pos(std::vector<u32>(want.size(), kFill));
        bitmap_positions(nullptr, (const uint64_t *)dv.p, (const uint64_t *)kp, n, prefix.p, pos.p, capacity, true);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        expect_equal(what + " positions capacity=" + std::to_string(capacity), pos.fetch(), want);
    }
    // without the sentinel nothing lands behind the last position
    std::vector<u32> want((size_t)total + 1 + kGuard, kFill);
    for (int64_t j = 0; j < total; j++) want[(size_t)j] = want_pos[(size_t)j];
    Dev<u32> pos(std::vector<u32>(want.size(), kFill));
    bitmap_positions(nullptr, (const uint64_t *)dv.p, (const uint64_t *)kp, n, prefix.p, pos.p, total, false);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    expect_equal(what + " positions no sentinel", pos.fetch(), want);
}

std::vector<u64> words_of_density(int64_t nw, int kind, u64 seed) {   // 0: all zero, 1: all one, 2: about 5 %, 3: about 50 %
    std::vector<u64> v((size_t)nw, kind == 1 ? ~0ull : 0ull);
    if (kind >= 2) {
        Lcg r{seed};
        for (auto &w : v)
            for (int b = 0; b < 64; b++)
                if (r.next() % 100u < (kind == 2 ? 5u : 50u)) w |= 1ull << b;
    }
    return v;
}

void bitmap_cases() {
    const int64_t ns[] = {1, 63, 64, 65, 4095, 4096, 4097, 64ll * 1024 * 64 + 37};
    const char *names[] = {"zeros", "ones", "5 percent"};
    for (int64_t n : ns) {
        const int64_t nw = (n + 63) / 64;
        for (int kind = 0; kind < 3; kind++)
            for (int masked = 0; masked < 2; masked++)
                bitmap_case(names[kind], n, words_of_density(nw, kind, (u64)n + 11), masked ? words_of_density(nw, 3, (u64)n + 5) : std::vector<u64>());
    }
    // past one sweep of the positions' capped grid (2048 blocks of 256 words): the strided loop takes a second trip
    const int64_t sweep = 2048ll * 256 * 64 + 3 * 64 + 5;
    bitmap_case("5 percent, second sweep", sweep, words_of_density((sweep + 63) / 64, 2, 77), {});
    // one wave's 64 words with exactly 1024 kept rows (staged through LDS) and with 1025 (stored directly)
    std::vector<u64> v(64, 0xFFFFull);
    bitmap_case("1024 in a wave", 4096, v, {});
    v[17] = 0x1FFFFull;
    bitmap_case("1025 in a wave", 4096, v, {});
}

}  // namespace

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        std::printf("test_scan: no GPU, and no CPU fallback\n");
        return 2;
    }
    carry_cases<u32, 256>();
    carry_cases<u32, 1024>();
    carry_cases<u64, 256>();
    carry_cases<u64, 1024>();
    carry_case<u64, 1024>(1024 + 1, 1, 1ull << 23, true);   // ~ 1000 * 2^23 * 1025: the running sum passes 2^32 many times over
    carry_case<u32, 1024>(3 * 1024 + 7, 3, 1, false);
    const int64_t ns[] = {1, 1023, 1024, 1025, 1024 * 1024 - 1, 1024 * 1024, 1024 * 1024 + 1025};
    for (int64_t n : ns)
        for (bool in_place : {false, true}) {
            exclusive_case<u32>(n, in_place);
            exclusive_case<i64>(n, in_place);
        }
    bitmap_cases();
    std::printf("scan primitives: all %d checks passed\n", g_checks);
    return 0;
}
