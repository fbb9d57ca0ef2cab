// ASan/UBSan driver for lc_amd/csrc/lc_sym_args.h (CPU only, its own main; run by hand, outside pytest):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/sym_args_sanitize.cpp -o sym_args_sanitize
// The argument rules of the symmetry entry points are plain host code that never dereferences a pointer.  Every pointer handed over
// here is the END of an exact-sized heap block (one byte past it is poisoned), so a rule that read through one would trip
// AddressSanitizer, and the size arithmetic is driven to its integer limits for UBSan.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../lc_amd/csrc/lc_sym_args.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("CHECK failed line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static bool has(const char* msg, const char* part) { return msg && std::strstr(msg, part); }

int main() {
    using namespace lc::host;
    char* block = (char*)std::malloc(64);
    const void* p = block + 64;  // 16-byte aligned (malloc), not one readable byte behind it
    const void* odd = block + 62;
    const void* half = block + 60;

    CHECK(!sym_select_size_error(1, 5, 64, 8, 8) && !sym_select_size_error(0, 0, 1, 0, 0));
    CHECK(has(sym_select_size_error(1, -1, 64, 8, 8), "size") && has(sym_select_size_error(1, 5, 0, 8, 8), "size"));
    CHECK(has(sym_select_size_error(1, INT_MAX, INT_MAX, INT_MAX, INT_MAX), "1024") && has(sym_select_size_error(2, 5, 64, 8, 8), "mode"));

    CHECK(!sym_select_points_error(0, p, p, p, nullptr, 0, 0, nullptr, nullptr, nullptr, 5, 0, 0, p));
    CHECK(has(sym_select_points_error(0, p, p, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 5, 0, 0, p), "2D"));
    CHECK(has(sym_select_points_error(1, nullptr, p, p, nullptr, 0, 0, nullptr, nullptr, nullptr, 5, 0, 0, p), "null"));
    CHECK(has(sym_select_points_error(1, p, nullptr, p, nullptr, 0, 0, nullptr, nullptr, p, 5, 8, 8, p), "noc_scale"));
    CHECK(has(sym_select_points_error(1, p, p, nullptr, nullptr, 0, 0, nullptr, nullptr, p, 5, 8, 8, p), "homo_z"));
    CHECK(has(sym_select_points_error(1, p, p, nullptr, nullptr, 0, 0, nullptr, p, nullptr, 5, 8, 8, p), "check pixels"));
    CHECK(has(sym_select_points_error(1, p, p, nullptr, nullptr, 0, 0, nullptr, p, p, 5, 0, 8, p), "map size"));
    CHECK(has(sym_select_points_error(1, p, p, nullptr, nullptr, 0, 0, nullptr, p, p, INT_MAX, INT_MAX, INT_MAX, p), "2^31"));
    CHECK(has(sym_select_points_error(1, p, nullptr, p, p, 3, 0, p, nullptr, p, 5, 8, 8, p), "map_dtype"));
    CHECK(has(sym_select_points_error(1, p, nullptr, p, p, 0, 10, p, nullptr, p, 5, 8, 8, p), "stride"));
    CHECK(has(sym_select_points_error(1, p, nullptr, p, p, 0, LLONG_MIN, p, nullptr, p, 5, 8, 8, p), "stride"));
    CHECK(!sym_select_points_error(1, p, nullptr, nullptr, p, 2, LLONG_MAX, p, p, p, 32, 256, 256, p));

    CHECK(!sym_table_error(p, p, p, p, p, 1, 1) && !sym_table_error(p, p, p, p, p, INT_MAX, 178956969));
    CHECK(has(sym_table_error(p, p, p, p, p, 0, 5), "at least one") && has(sym_table_error(p, p, p, p, p, 3, INT_MIN), "at least one"));
    CHECK(has(sym_table_error(p, p, p, p, p, 3, INT_MAX), "2^31") && has(sym_table_error(p, p, p, p, p, 3, 178956970), "2^31"));
    CHECK(has(sym_table_error(p, p, nullptr, p, p, 3, 5), "null") && has(sym_table_error(nullptr, p, p, p, p, 3, 5), "null"));
    CHECK(has(sym_table_error(p, p, half, p, p, 3, 5), "8-byte") && has(sym_table_error(p, odd, p, p, p, 3, 5), "4-byte"));
    CHECK(!sym_table_error(half, half, p, half, half, 3, 5));

    CHECK(!sym_candidates_out_error(p, p, 40) && !sym_candidates_out_error(half, half, 178956969));
    CHECK(has(sym_candidates_out_error(p, p, 0), "out_rows") && has(sym_candidates_out_error(p, p, INT_MAX), "out_rows"));
    CHECK(has(sym_candidates_out_error(nullptr, p, 40), "null") && has(sym_candidates_out_error(p, odd, 40), "4-byte"));
    CHECK(has(sym_candidates_out_error(odd, p, 40), "row_off"));

    std::free(block);
    if (failures) std::printf("FAILED (%d)\n", failures);
    else std::printf("sym_args_sanitize: all checks passed\n");
    return failures ? 1 : 0;
}
