// The two decisions of a PSF pass (csrc/svr_plan.h: pass_path, table_plan) enumerated on the host: no engine, no GPU.
// Run by tests/test_plan_cpu.py; exits 0 when every expectation holds, prints the first one that does not.  The expectations are literal.
#include <cstdio>

#include "../fetalreconstruction_amd/csrc/svr_plan.h"

static const Pass PASSES[] = {PASS_GAUSS1, PASS_GAUSS2, PASS_FORWARD, PASS_BACK, PASS_BIAS, PASS_CHANNEL_SCATTER, PASS_CHANNEL_GATHER};
static const char *const PASS_NAMES[] = {"gauss1", "gauss2", "forward", "back", "bias", "channel scatter", "channel gather"};
static const char *const USE_NAMES[] = {"evaluate", "stream", "store"};

// ---- (a) pass_path -------------------------------------------------------------------------------------------------------------
// the options in PassOptions' order: pvr, pvr_mode, back_mode, fwd_mode, gauss_mode, bias_mode, fwd_mode_user, density, gather cell area
static const Family C = FAM_CELLS, T = FAM_TILES, X = FAM_PIXELS;
static const struct PathCase {
  const char *name;
  PassOptions o;
  PassPath want[5];        // gauss1, gauss2, forward, back, bias: {family, scatter_level, may_stream_table, table_on_cells}
} PATH_CASES[] = {
    {"SVR defaults, density 0.72", {0, 1, 5, 2, 1, 1, false, 0.72, 54}, {{C, 4, true, false}, {C, 4, true, false}, {C, 0, true, true}, {C, 4, true, false}, {C, 0, true, false}}},
    {"SVR density 0.65", {0, 1, 5, 2, 1, 1, false, 0.65, 54}, {{C, 4, true, false}, {C, 4, true, false}, {C, 0, true, true}, {C, 4, true, false}, {C, 0, true, false}}},
    {"SVR density 0.64", {0, 1, 5, 2, 1, 1, false, 0.64, 200}, {{C, 4, true, false}, {C, 4, true, false}, {C, 0, true, false}, {C, 4, true, false}, {C, 0, true, false}}},
    {"SVR density 0.5, fwd_mode by the caller", {0, 1, 5, 2, 1, 1, true, 0.5, 54}, {{C, 4, true, false}, {C, 4, true, false}, {C, 0, true, true}, {C, 4, true, false}, {C, 0, true, false}}},
    {"PVR defaults, gather cells of 96", {1, 1, 5, 2, 1, 1, false, 0.3, 96}, {{C, 4, true, false}, {C, 4, true, false}, {C, 0, true, true}, {C, 4, true, false}, {X, 0, false, false}}},
    {"PVR defaults, gather cells of 95", {1, 1, 5, 2, 1, 1, false, 0.9, 95}, {{C, 4, true, false}, {C, 4, true, false}, {C, 0, true, false}, {C, 4, true, false}, {X, 0, false, false}}},
    {"PVR gather cells of 10, fwd_mode by the caller", {1, 1, 5, 2, 1, 1, true, 0.3, 10}, {{C, 4, true, false}, {C, 4, true, false}, {C, 0, true, true}, {C, 4, true, false}, {X, 0, false, false}}},
    {"back_mode 4, fwd_mode 1", {0, 1, 4, 1, 1, 1, true, 0.72, 54}, {{T, 4, true, false}, {T, 4, true, false}, {T, 0, true, true}, {T, 4, true, false}, {X, 0, false, false}}},
    {"PVR back_mode 4, fwd_mode 1", {1, 1, 4, 1, 1, 1, false, 0.72, 54}, {{T, 4, true, false}, {T, 4, true, false}, {T, 0, true, false}, {T, 4, true, false}, {X, 0, false, false}}},
    {"back_mode 0", {0, 1, 0, 2, 1, 1, false, 0.72, 54}, {{C, 1, true, false}, {T, 1, true, false}, {C, 0, true, true}, {X, 0, false, false}, {X, 0, false, false}}},
    {"back_mode 1", {0, 1, 1, 2, 1, 1, false, 0.72, 54}, {{C, 1, true, false}, {T, 1, true, false}, {C, 0, true, true}, {T, 1, false, false}, {X, 0, false, false}}},
    {"back_mode 3", {0, 1, 3, 2, 1, 1, false, 0.72, 54}, {{C, 3, true, false}, {T, 3, true, false}, {C, 0, true, true}, {T, 3, false, false}, {X, 0, false, false}}},
    {"fwd_mode 0", {0, 1, 5, 0, 1, 1, true, 0.72, 54}, {{T, 4, true, false}, {C, 4, true, false}, {X, 0, false, false}, {C, 4, true, false}, {C, 0, true, false}}},
    {"gauss_mode 0", {0, 1, 5, 2, 0, 1, false, 0.72, 54}, {{X, 0, false, false}, {X, 0, false, false}, {C, 0, true, true}, {C, 4, true, false}, {C, 0, true, false}}},
    {"PVR pvr_mode 0", {1, 0, 5, 2, 1, 1, false, 0.72, 200}, {{X, 0, false, false}, {X, 0, false, false}, {X, 0, false, false}, {X, 0, false, false}, {X, 0, false, false}}},
    {"bias_mode 0", {0, 1, 5, 2, 1, 0, false, 0.72, 54}, {{C, 4, true, false}, {C, 4, true, false}, {C, 0, true, true}, {C, 4, true, false}, {X, 0, false, false}}},
};

static bool same(const PassPath &a, const PassPath &b) {
  return a.family == b.family && a.scatter_level == b.scatter_level && a.may_stream_table == b.may_stream_table && a.table_on_cells == b.table_on_cells;
}
static int check_paths() {
  for (const PathCase &c : PATH_CASES)
    for (int i = 0; i < 5; ++i) {
      const PassPath p = pass_path(c.o, PASSES[i]), &w = c.want[i];
      if (!same(p, w)) {
        std::printf("pass_path, %s, %s: family %d level %d stream %d on_cells %d, expected %d %d %d %d\n", c.name, PASS_NAMES[i], p.family, p.scatter_level,
                    p.may_stream_table, p.table_on_cells, w.family, w.scatter_level, w.may_stream_table, w.table_on_cells);
        return 1;
      }
    }
  // a channel's passes take the SR passes' paths
  for (const PathCase &c : PATH_CASES)
    if (!same(pass_path(c.o, PASS_CHANNEL_SCATTER), c.want[3]) || !same(pass_path(c.o, PASS_CHANNEL_GATHER), c.want[2])) {
      std::printf("pass_path, %s: a channel pass differs from the SR pass\n", c.name);
      return 1;
    }
  return 0;
}

// ---- (b) table_plan ------------------------------------------------------------------------------------------------------------
// A row: a pattern over (may_stream_table, table_on_cells, wanted, state N / P / F, lazy_ok, cells usable, active pixels, PSF pixels), '*' = any.
// The first row of the pass that matches a combination says its plan; a combination that no row matches evaluates and builds nothing.
static struct PlanRow {
  Pass pass;
  const char *pat;
  bool build_first;
  TableUse use;
  int hits;
} PLAN_ROWS[] = {
    // the Gaussian reconstruction: one decision for both passes.  Streams a FULL table only; pending -> pass 2 stores on its cells
    {PASS_GAUSS1, "**1N111*", false, TABLE_STORE, 0},
    {PASS_GAUSS1, "1*1N0*1*", true, TABLE_STREAM, 0},
    {PASS_GAUSS1, "1*1F****", false, TABLE_STREAM, 0},
    {PASS_GAUSS2, "**1N111*", false, TABLE_STORE, 0},
    {PASS_GAUSS2, "1*1N0*1*", true, TABLE_STREAM, 0},
    {PASS_GAUSS2, "1*1F****", false, TABLE_STREAM, 0},
    // forward: stores a pending table on usable gather cells, else builds whatever is absent -- lazy or not, streaming or not
    {PASS_FORWARD, "**1N1111", false, TABLE_STORE, 0},
    {PASS_FORWARD, "1*1N**1*", true, TABLE_STREAM, 0},
    {PASS_FORWARD, "0*1N**1*", true, TABLE_EVALUATE, 0},
    {PASS_FORWARD, "1*1P****", false, TABLE_STREAM, 0},
    {PASS_FORWARD, "1*1F****", false, TABLE_STREAM, 0},
    // back: stores a pending table on usable cells; a pending table it cannot store stays absent; builds only what is not lazy
    {PASS_BACK, "**1N1111", false, TABLE_STORE, 0},
    {PASS_BACK, "1*1N0*1*", true, TABLE_STREAM, 0},
    {PASS_BACK, "0*1N0*1*", true, TABLE_EVALUATE, 0},
    {PASS_BACK, "1*1P****", false, TABLE_STREAM, 0},
    {PASS_BACK, "1*1F****", false, TABLE_STREAM, 0},
    // the cell-only readers
    {PASS_BIAS, "**1P****", false, TABLE_STREAM, 0},
    {PASS_BIAS, "**1F****", false, TABLE_STREAM, 0},
    {PASS_CHANNEL_SCATTER, "**1P****", false, TABLE_STREAM, 0},
    {PASS_CHANNEL_SCATTER, "**1F****", false, TABLE_STREAM, 0},
    {PASS_CHANNEL_GATHER, "111P****", false, TABLE_STREAM, 0},
    {PASS_CHANNEL_GATHER, "111F****", false, TABLE_STREAM, 0},
};

static int check_plans() {
  static const char STATES[] = "NPF";
  static const bool LISTS[3][2] = {{false, false}, {true, false}, {true, true}};   // {active pixels, PSF pixels}: the PSF pixels are active pixels
  int evaluated = 0;
  for (int ip = 0; ip < 7; ++ip)
    for (int bits = 0; bits < 32; ++bits)
      for (int st = 0; st < 3; ++st)
        for (int li = 0; li < 3; ++li) {
          const bool stream = bits & 1, on_cells = bits & 2, wanted = bits & 4, lazy = bits & 8, cells = bits & 16;
          const char key[9] = {stream ? '1' : '0', on_cells ? '1' : '0', wanted ? '1' : '0', STATES[st], lazy ? '1' : '0', cells ? '1' : '0',
                               LISTS[li][0] ? '1' : '0', LISTS[li][1] ? '1' : '0', 0};
          TablePlan want = {false, TABLE_EVALUATE};
          PlanRow *row = nullptr;
          for (PlanRow &r : PLAN_ROWS) {
            if (r.pass != PASSES[ip]) continue;
            bool m = true;
            for (int k = 0; k < 8; ++k) m = m && (r.pat[k] == '*' || r.pat[k] == key[k]);
            if (m) { row = &r; break; }
          }
          if (row) { want.build_first = row->build_first; want.use = row->use; ++row->hits; } else ++evaluated;
          const PassPath p = {FAM_CELLS, 0, stream, on_cells};
          const TableInputs t = {wanted, (CoeffState)st, lazy, LISTS[li][0], LISTS[li][1], cells};
          const TablePlan got = table_plan(PASSES[ip], p, t);
          if (got.build_first != want.build_first || got.use != want.use) {
            std::printf("table_plan, %s, %s: build_first %d, %s; expected %d, %s (row %s)\n", PASS_NAMES[ip], key, got.build_first, USE_NAMES[got.use],
                        want.build_first, USE_NAMES[want.use], row ? row->pat : "none");
            return 1;
          }
          if (got.use == TABLE_STORE && got.build_first) { std::printf("table_plan, %s, %s: stores what it built first\n", PASS_NAMES[ip], key); return 1; }
          // off the cell kernels the lists' word counts for nothing: as if they were unusable
          for (Family f : {FAM_TILES, FAM_PIXELS}) {
            const PassPath pf = {f, 0, stream, on_cells};
            TableInputs tf = t;
            tf.cells_usable = false;
            const TablePlan a = table_plan(PASSES[ip], pf, t), b = table_plan(PASSES[ip], p, tf);
            if (a.build_first != b.build_first || a.use != b.use) { std::printf("table_plan, %s, %s: family %d and unusable cells differ\n", PASS_NAMES[ip], key, f); return 1; }
          }
        }
  for (const PlanRow &r : PLAN_ROWS)
    if (!r.hits) { std::printf("table_plan: row %s of %s matched nothing\n", r.pat, PASS_NAMES[r.pass]); return 1; }
  // 7 passes x 288 combinations; the rows take 40 + 40 (Gaussian), 80 (forward), 68 (back), 96 + 96 (bias, channel scatter), 24 (channel gather)
  if (evaluated != 2016 - 444) { std::printf("table_plan: %d combinations outside the rows, expected %d\n", evaluated, 2016 - 444); return 1; }
  return 0;
}

static int check_gather_stays() {
  static const struct { bool on_cells; TableUse use; bool want; } rows[] = {
      {false, TABLE_EVALUATE, true}, {false, TABLE_STORE, true}, {false, TABLE_STREAM, false},
      {true, TABLE_EVALUATE, true},  {true, TABLE_STORE, true},  {true, TABLE_STREAM, true}};
  for (const auto &r : rows) {
    const PassPath p = {FAM_CELLS, 0, true, r.on_cells};
    if (gather_stays_on_cells(p, r.use) != r.want) { std::printf("gather_stays_on_cells(table_on_cells %d, %s) is not %d\n", r.on_cells, USE_NAMES[r.use], r.want); return 1; }
  }
  return 0;
}

int main() {
  if (check_paths() || check_plans() || check_gather_stays()) return 1;
  std::printf("ok\n");
  return 0;
}
