/* headroom_host_helpers.c — the shared routines behind libykhost's headroom calls (host.cpp: headroom_list, headroom_rows,
 * ask_row_by_key, headroom_by_key) on a MIRROR-ONLY handle (device -1), for a build of libykhost's sources under AddressSanitizer +
 * UBSan (tests/test_headroom_host_helpers.py). What a handle without an engine reaches: the argument checks, the unknown key, the
 * pod that holds no ask row, and the mirror-only answer — with the output cells every call promises on those paths. The index check
 * and the routed answer lie behind the engine's tables and belong to the GPU suite.
 * Exit code 0 and "headroom helpers ok" = every call behaved. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ykhost.h"

static int failures = 0;
#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                   \
    }                                                               \
  } while (0)

typedef int32_t (*list_fn)(ykhost_t*, int32_t, const int32_t*, int64_t*);
typedef int32_t (*rows_fn)(ykhost_t*, int32_t, int64_t*, int64_t*, int32_t, char*, int64_t);
typedef int32_t (*key_fn)(ykhost_t*, const char*, int64_t*, char*, int64_t);

static int32_t plain_by_key(ykhost_t* h, const char* key, int64_t* out16, char* best, int64_t best_len) {
  (void)best, (void)best_len;
  return ykhost_headroom_by_key(h, key, out16);
}
static int error_is(ykhost_t* h, const char* text) { return strcmp(ykhost_last_error(h), text) == 0; }
static int all_zero(const int64_t* c, int n) {
  for (int i = 0; i < n; ++i)
    if (c[i]) return 0;
  return 1;
}

static const char* kMirrorOnly = "mirror-only handle (device < 0): no device engine, nothing can be evaluated";

int main(void) {
  char err[256];
  ykhost_t* h = ykhost_create(-1, err, sizeof err);
  if (!h) {
    fprintf(stderr, "ykhost_create: %s\n", err);
    return 1;
  }
  EXPECT(ykhost_update_node(h, "{\"kind\":\"Node\",\"apiVersion\":\"v1\",\"metadata\":{\"name\":\"node-a\",\"labels\":{\"kubernetes.io/hostname\":\"node-a\"}},"
                               "\"spec\":{},\"status\":{\"allocatable\":{\"cpu\":\"4\",\"memory\":\"8Gi\",\"pods\":\"10\"}}}") == 0);
  const char* pod = "{\"kind\":\"Pod\",\"apiVersion\":\"v1\",\"metadata\":{\"name\":\"%s\",\"namespace\":\"default\",\"uid\":\"%s\"},\"spec\":{\"containers\":[{\"name\":\"c\","
                    "\"resources\":{\"requests\":{\"cpu\":\"1\"}}}],\"schedulerName\":\"yunikorn\"%s},\"status\":{\"phase\":\"%s\"}}";
  char doc[1024];
  snprintf(doc, sizeof doc, pod, "running-1", "running-1", ",\"nodeName\":\"node-a\"", "Running");
  EXPECT(ykhost_update_pod(h, doc) == 1);
  snprintf(doc, sizeof doc, pod, "ask-1", "ask-1", "", "Pending");
  EXPECT(ykhost_update_pod(h, doc) == 1);

  const char* names[3] = {"headroom", "headroom_spread", "headroom_affinity"};
  const list_fn lists[3] = {ykhost_headroom, ykhost_headroom_spread, ykhost_headroom_affinity};
  const key_fn keys[3] = {plain_by_key, ykhost_headroom_spread_by_key, ykhost_headroom_affinity_by_key};
  const rows_fn rows[3] = {NULL, ykhost_headroom_spread_domains, ykhost_headroom_affinity_domains};
  for (int v = 0; v < 3; ++v) {
    char want[128];
    int64_t* cells = (int64_t*)malloc(2 * 16 * sizeof(int64_t)); /* (exactly the cells of two asks: a write past them is a report) */
    const int32_t asks[2] = {0, 7};
    /* the list call: bad arguments, then the mirror-only answer (before any index is looked at) */
    snprintf(want, sizeof want, "%s: bad argument", names[v]);
    EXPECT(lists[v](h, -1, asks, cells) == -1 && error_is(h, want));
    EXPECT(lists[v](h, 2, asks, NULL) == -1 && error_is(h, want));
    EXPECT(lists[v](h, 2, asks, cells) == YKPRED_E_STATE && error_is(h, kMirrorOnly));
    EXPECT(lists[v](h, 0, NULL, NULL) == YKPRED_E_STATE && error_is(h, kMirrorOnly));
    /* one ask by its allocation key */
    char* best = (char*)malloc(8);
    snprintf(want, sizeof want, "%s_by_key: bad argument", names[v]);
    EXPECT(keys[v](h, "ask-1", NULL, best, 8) == -1 && error_is(h, want));
    memset(cells, 0x55, 16 * sizeof(int64_t));
    strcpy(best, "stale");
    EXPECT(keys[v](h, "no-such-pod", cells, best, 8) == YKHOST_E_POD_NOT_FOUND && all_zero(cells, 16) && (v == 0 || best[0] == 0));
    EXPECT(keys[v](h, NULL, cells, NULL, 0) == YKHOST_E_POD_NOT_FOUND);
    memset(cells, 0x55, 16 * sizeof(int64_t));
    EXPECT(keys[v](h, "running-1", cells, best, 8) == YKHOST_E_NOT_AN_ASK && error_is(h, "pod holds no ask row") && all_zero(cells, 16));
    memset(cells, 0x55, 16 * sizeof(int64_t));
    EXPECT(keys[v](h, "ask-1", cells, best, 8) == YKPRED_E_STATE && error_is(h, kMirrorOnly) && all_zero(cells, 16));
    free(best);
    /* the per-domain rows of one ask */
    if (rows[v]) {
      int64_t* table = (int64_t*)malloc(3 * 4 * sizeof(int64_t));
      char* values = (char*)malloc(4);
      snprintf(want, sizeof want, "%s_domains: bad argument", names[v]);
      EXPECT(rows[v](h, 0, NULL, table, 2, values, 4) == -1 && error_is(h, want));
      EXPECT(rows[v](h, 0, cells, table, -1, values, 4) == -1 && error_is(h, want));
      EXPECT(rows[v](h, 0, cells, NULL, 2, values, 4) == -1 && error_is(h, want));
      /* (no rows asked for: the spread call takes no table, the affinity call always writes the outside row) */
      strcpy(values, "xx");
      const int32_t rc = rows[v](h, 0, cells, NULL, 0, values, 4);
      EXPECT(v == 1 ? (rc == YKPRED_E_STATE && error_is(h, kMirrorOnly) && strcmp(values, "[]") == 0) : (rc == -1 && error_is(h, want)));
      strcpy(values, "xx");
      EXPECT(rows[v](h, 0, cells, table, 2, values, 4) == YKPRED_E_STATE && error_is(h, kMirrorOnly) && strcmp(values, "[]") == 0);
      EXPECT(rows[v](h, 0, cells, table, 2, NULL, 0) == YKPRED_E_STATE);
      free(values);
      free(table);
    }
    free(cells);
  }
  /* the domain call by key shares the lookup */
  {
    int64_t* sum = (int64_t*)malloc(8 * sizeof(int64_t));
    char best[8] = "stale", tight[8] = "stale";
    EXPECT(ykhost_headroom_domain_by_key(h, "no-such-pod", "zone", 1, sum, best, 8, tight, 8) == YKHOST_E_POD_NOT_FOUND && all_zero(sum, 8) && !best[0] && !tight[0]);
    EXPECT(ykhost_headroom_domain_by_key(h, "running-1", "zone", 1, sum, best, 8, tight, 8) == YKHOST_E_NOT_AN_ASK);
    EXPECT(ykhost_headroom_domain_by_key(h, "ask-1", "zone", 1, sum, best, 8, tight, 8) == YKPRED_E_STATE && error_is(h, kMirrorOnly) && all_zero(sum, 8));
    free(sum);
  }
  ykhost_destroy(h);
  if (!failures) printf("headroom helpers ok\n");
  return failures ? 1 : 0;
}
