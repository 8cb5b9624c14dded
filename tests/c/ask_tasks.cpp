/* ask_tasks.cpp — the host side every per-ask query of the engine shares (csrc/engine/ask_tasks.h: the partition of a list of asks into
 * tasks, the two agreement words, the fix-up of a packed best key), for a build under AddressSanitizer + UBSan
 * (tests/test_ask_tasks_cpu.py). No device is touched and no library is linked.
 *
 *   ask_tasks <cases file>
 * Every line of the file is one case and every case prints one line:
 *   P  sharded by_ask with_extra  P  spec[P] pin[P]  n  asks[n] (extra[n])  →  T  task_of[n]  spec[T] pin[T]  E extra_of[E]  list partition
 *   K  cells at key limit row[cells]                                       →  row[cells]
 * Exit code 0 and a last line "ask tasks ok" = every case was read. */
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../yunikorn-k8shim_amd/csrc/engine/ask_tasks.h"

static bool read_ints(FILE* f, std::vector<int32_t>* v, size_t n) {
  v->assign(n, 0);  // (exactly n: a read or write past a table is caught)
  for (auto& x : *v)
    if (fscanf(f, "%" SCNd32, &x) != 1) return false;
  return true;
}

static void print_ints(const std::vector<int32_t>& v) {
  for (const int32_t x : v) printf(" %" PRId32, x);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char kind = 0;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'P') {
      int sharded = 0, by_ask = 0, with_extra = 0, P = 0, n = 0;
      std::vector<int32_t> spec, pin, asks, extra;
      if (fscanf(f, "%d %d %d %d", &sharded, &by_ask, &with_extra, &P) != 4 || !read_ints(f, &spec, (size_t)P) || !read_ints(f, &pin, (size_t)P) ||
          fscanf(f, "%d", &n) != 1 || !read_ints(f, &asks, (size_t)n) || (with_extra && !read_ints(f, &extra, (size_t)n)))
        return 2;
      yktasks::Partition part;
      part.task_of.assign(5, 77);  // (stale contents of an earlier call must not survive)
      part.spec.assign(3, 77);
      part.extra_of.assign(2, 77);
      yktasks::partition(spec.data(), pin.data(), n, n ? asks.data() : nullptr, with_extra ? extra.data() : nullptr, sharded != 0, by_ask != 0, &part);
      uint64_t list = 0, words = 0;
      yktasks::agreement_words(n, asks.data(), part.task_of.data(), &list, &words);
      printf("%zu", part.spec.size());
      print_ints(part.task_of);
      print_ints(part.spec);
      print_ints(part.pin);
      printf(" %zu", part.extra_of.size());
      print_ints(part.extra_of);
      printf(" %" PRIu64 " %" PRIu64 "\n", list, words);
    } else if (kind == 'K') {
      int cells = 0, at = 0;
      unsigned long long key = 0;
      long long limit = 0;
      if (fscanf(f, "%d %d %llu %lld", &cells, &at, &key, &limit) != 4) return 2;
      std::vector<int64_t> row((size_t)cells);
      for (auto& c : row) {
        long long v = 0;
        if (fscanf(f, "%lld", &v) != 1) return 2;
        c = v;
      }
      yktasks::best_key_fixup(row.data(), cells, at, (uint64_t)key, limit);
      for (size_t c = 0; c < row.size(); ++c) printf("%" PRId64 "%c", row[c], c + 1 == row.size() ? '\n' : ' ');
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("ask tasks ok\n");
  return 0;
}
