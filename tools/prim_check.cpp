// The carved form of the rocPRIM wrapper (csrc/gs_scratch.h: gs_prim_carved) against stand-in calls, host only: a call
// that needs more than the room it is given is refused with GS_ERR_DEVICE and a message naming the site, and is never
// invoked with a temporary; one that fits runs once with the temporary and its own need; a failing query or run is
// GS_ERR_DEVICE with the site's name.  Built and run by `make prim-check` under the address and undefined-behaviour
// sanitizers.
#include "gs_scratch.h"

#include <cstdio>
#include <cstdlib>

static std::string g_error;
void gs_set_error(const std::string &s) { g_error = s; }

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "prim_check: line %d: %s\n", __LINE__, #cond);   \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

struct stand_in {
  size_t need;
  hipError_t query_result = hipSuccess, run_result = hipSuccess;
  int queries = 0, runs = 0;
  void *ran_with = nullptr;
  size_t ran_bytes = 0;
  hipError_t operator()(void *tmp, size_t &bytes) {
    if (!tmp) {
      queries++;
      bytes = need;
      return query_result;
    }
    runs++;
    ran_with = tmp;
    ran_bytes = bytes;
    return run_result;
  }
};

int main() {
  char room[64];
  for (size_t need : {(size_t)65, (size_t)1 << 40}) { /* a shortfall of one byte, and a large one */
    stand_in c{need};
    g_error.clear();
    CHECK(gs_prim_carved("the site's name", room, sizeof room, c) == GS_ERR_DEVICE);
    CHECK(c.queries == 1 && c.runs == 0);
    CHECK(g_error.find("the site's name") != std::string::npos && g_error.find(std::to_string(need)) != std::string::npos &&
          g_error.find("64") != std::string::npos);
  }
  for (size_t need : {(size_t)0, (size_t)1, (size_t)64}) { /* up to the room exactly */
    stand_in c{need};
    CHECK(gs_prim_carved("fits", room, sizeof room, c) == GS_OK);
    CHECK(c.queries == 1 && c.runs == 1 && c.ran_with == room && c.ran_bytes == need);
  }
  { /* no temporary at all is no run either */
    stand_in c{8};
    CHECK(gs_prim_carved("no temporary", nullptr, 64, c) == GS_ERR_DEVICE && c.runs == 0);
  }
  { /* the query fails: nothing runs */
    stand_in c{8};
    c.query_result = hipErrorInvalidValue;
    g_error.clear();
    CHECK(gs_prim_carved("query", room, sizeof room, c) == GS_ERR_DEVICE && c.runs == 0);
    CHECK(g_error.find("query: ") == 0);
  }
  { /* the run fails */
    stand_in c{8};
    c.run_result = hipErrorInvalidValue;
    g_error.clear();
    CHECK(gs_prim_carved("run", room, sizeof room, c) == GS_ERR_DEVICE && c.runs == 1);
    CHECK(g_error.find("run: ") == 0);
  }
  { /* a lambda, as the call sites write it */
    int runs = 0;
    CHECK(gs_prim_carved("lambda", room, 16, [&](void *t, size_t &b) {
            if (!t) b = 17;
            else runs++;
            return hipSuccess;
          }) == GS_ERR_DEVICE && runs == 0);
  }
  printf("prim_check: ok\n");
  return 0;
}
