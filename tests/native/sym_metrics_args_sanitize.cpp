// ASan/UBSan driver for lc_amd/csrc/symerr/lc_sym_metrics_args.h (CPU only, its own main; tests/test_symerr_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/sym_metrics_args_sanitize.cpp -o sym_metrics_args_sanitize
// The argument rules of lc_sym_pose_errors_f32 are plain host code that never dereferences a pointer.  Every pointer handed over here is the
// END of an exact-sized heap block (one byte past it is poisoned), so a rule that read through one would trip AddressSanitizer, and the
// size arithmetic is driven to its integer limits for UBSan.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../lc_amd/csrc/lc_sym_args.h"
#include "../../lc_amd/csrc/symerr/lc_sym_metrics_args.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("CHECK failed line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static bool has(const char* msg, const char* part) { return msg && std::strstr(msg, part); }

int main() {
    using namespace lc::host;
    char* block = (char*)std::malloc(64);
    const void* p = block + 64;  // 16-byte aligned (malloc), not one readable byte behind it
    const void* odd = block + 62;
    const void* half = block + 60;

    CHECK(sym_errors_chunks(1) == 1 && sym_errors_chunks(8) == 1 && sym_errors_chunks(9) == 2 && sym_errors_chunks(INT_MAX) == 268435456ll);
    CHECK(sym_errors_workspace_bytes(0, 5) == 0 && sym_errors_workspace_bytes(5, 0) == 0 && sym_errors_workspace_bytes(-1, -1) == 0);
    CHECK(sym_errors_workspace_bytes(1, 1) == 24 && sym_errors_workspace_bytes(64, 768) == 64u * (2 * 96 + 1) * 8);
    CHECK(sym_errors_workspace_bytes(INT_MAX, INT_MAX) == (size_t)INT_MAX * (2 * (size_t)268435456 + 1) * 8);

    CHECK(!sym_errors_size_error(0, 0, 0) && !sym_errors_size_error(64, 5000, 768) && !sym_errors_size_error(7, 715827881, 8));
    CHECK(has(sym_errors_size_error(-1, 5, 5), "size") && has(sym_errors_size_error(1, -5, 5), "size") && has(sym_errors_size_error(1, 5, INT_MIN), "size"));
    CHECK(has(sym_errors_size_error(1, 715827882, 5), "2^31") && has(sym_errors_size_error(1, INT_MAX, 5), "2^31"));
    CHECK(has(sym_errors_size_error(INT_MAX, 5, INT_MAX), "chunks") && has(sym_errors_size_error(1073741824, 5, 9), "chunks"));
    CHECK(!sym_errors_size_error(1073741823, 5, 9) && !sym_errors_size_error(INT_MAX, 5, 8));

    auto args = [&](const void* Re, const void* te, const void* Rg, const void* tg, const void* K, const void* pts, const void* off, const void* cnt,
                    const void* err, const void* arg, const void* ws, size_t bytes, int P = 700, int max_k = 36, int B = 12) {
        return sym_errors_args_error(Re, te, Rg, tg, K, pts, off, cnt, P, max_k, B, err, arg, ws, bytes);
    };
    const size_t need = sym_errors_workspace_bytes(12, 36);
    CHECK(need == 12 * (2 * 5 + 1) * 8);
    CHECK(!args(p, p, p, p, p, p, p, p, p, p, p, need) && !args(half, half, half, half, half, half, nullptr, nullptr, half, half, p, need + 1));
    CHECK(has(args(p, p, p, p, p, p, p, p, p, p, p, need, 0), "at least one vertex") && has(args(p, p, p, p, p, p, p, p, p, p, p, need, 700, 0), "max_k"));
    CHECK(has(args(nullptr, p, p, p, p, p, p, p, p, p, p, need), "null") && has(args(p, p, p, p, nullptr, p, p, p, p, p, p, need), "null"));
    CHECK(has(args(p, p, p, p, p, nullptr, p, p, p, p, p, need), "null") && has(args(p, p, p, p, p, p, p, p, p, nullptr, p, need), "null"));
    CHECK(has(args(p, p, p, p, p, p, p, nullptr, p, p, p, need), "go together") && has(args(p, p, p, p, p, p, nullptr, p, p, p, p, need), "go together"));
    CHECK(has(args(p, odd, p, p, p, p, p, p, p, p, p, need), "4-byte") && has(args(p, p, p, p, p, p, p, odd, p, p, p, need), "4-byte"));
    CHECK(has(args(p, p, p, p, p, p, p, p, odd, p, p, need), "4-byte") && has(args(p, p, p, p, p, p, p, p, p, p, nullptr, need), "null workspace"));
    CHECK(has(args(p, p, p, p, p, p, p, p, p, p, half, need), "8-byte") && has(args(p, p, p, p, p, p, p, p, p, p, p, need - 1), "smaller"));
    CHECK(has(args(p, p, p, p, p, p, p, p, p, p, p, (size_t)-1 / 2, 700, INT_MAX, INT_MAX), "smaller"));

    // the table's rules as lc_sym_pose_errors_f32 applies them: the ground-truth rotations stand where the base pose stands
    CHECK(!sym_table_error(p, p, p, p, p, 4, 43) && has(sym_table_error(p, p, half, p, p, 4, 43), "8-byte") && has(sym_table_error(p, nullptr, p, p, p, 4, 43), "null"));

    std::free(block);
    if (failures) std::printf("FAILED (%d)\n", failures);
    else std::printf("sym_metrics_args_sanitize: all checks passed\n");
    return failures ? 1 : 0;
}
