// witness_status (csrc/rpsetup.hpp), the one host function behind every BPPP_RP_WIT_* verdict of the host-buffer prover routes, under
// AddressSanitizer / UndefinedBehaviorSanitizer on the shapes of examples/rec_test (typed: 1 + in1 + in2 = out, all of type 15) and
// examples/bin_test (conserved binary: 2 + in1 + in2 = out): every reason, the order of precedence (typed: canonical, balance, range — the lowest
// code that applies; binary: the first offending range, its blinding before its bounds, then the balance) and per-proof public amounts.
#include <cstdio>
#include <string>
#include <vector>
#include "rpsetup.hpp"
using namespace bppp_rps;
using bppp_host::U256;

static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad < 10) { printf(__VA_ARGS__); printf("\n"); } bad++; } } while (0)

static U256 from_i64(long long v) { return v < 0 ? u_sub(U256::zero(), U256::from_u64((uint64_t)(-v))) : U256::from_u64((uint64_t)v); }
static U256 pow2(int k) { U256 r = U256::zero(); r.w[k >> 6] = 1ull << (k & 63); return r; }
struct Row { std::vector<uint64_t> amt, typ, bld; };
static Row row(const std::vector<U256> &a, const std::vector<U256> &t, const std::vector<U256> &b) {
  Row r;
  r.amt.resize(4 * a.size()); r.typ.resize(4 * a.size()); r.bld.resize(4 * a.size());
  for (size_t i = 0; i < a.size(); i++) { a[i].store(&r.amt[4 * i]); t[i].store(&r.typ[4 * i]); b[i].store(&r.bld[4 * i]); }
  return r;
}
static uint32_t status(const Setup &st, const Row &r, const U256 *pub = nullptr) {
  uint64_t p[4];
  if (pub) pub->store(p);
  return witness_status(st, r.amt.data(), st.kind == 1 ? nullptr : r.typ.data(), r.bld.data(), pub ? p : nullptr);
}

int main() {
  std::string err;
  const U256 N = bppp_host::FR().m, t15 = U256::from_u64(15), one = U256::one();
  // ---- rec_test
  std::vector<RangeData> rds(3);
  CHECK(make_range_data(3, U256::zero(), pow2(64), true, true, false, rds[0], err), "range 0: %s", err.c_str());
  CHECK(make_range_data(16, from_i64(-20), u_sub(pow2(66), one), true, false, false, rds[1], err), "range 1: %s", err.c_str());
  CHECK(make_range_data(5, one, U256::from_u64(625), false, false, true, rds[2], err), "range 2: %s", err.c_str());
  Setup st;
  CHECK(make_setup(true, rds, {PublicVT{false, t15, one}}, st, err, 0), "rec_test: %s", err.c_str());
  const std::vector<U256> ty(3, t15), bl = {U256::from_u64(7), U256::from_u64(8), U256::from_u64(9)};
  auto typed = [&](long long out, long long in1, long long in2) { return row({from_i64(out), from_i64(in1), from_i64(in2)}, ty, bl); };
  CHECK(status(st, typed(131, 100, 30)) == WIT_OK, "a balanced witness refused");
  CHECK(status(st, typed(0, -20, 19)) == WIT_OK, "the minima refused");
  CHECK(status(st, typed(10, -21, 30)) == WIT_OUT_OF_RANGE, "in1 below its range");
  CHECK(status(st, typed(-1, -7, 5)) == WIT_OUT_OF_RANGE, "the output below 0");
  CHECK(status(st, row({pow2(64), u_sub(pow2(64), U256::from_u64(31)), U256::from_u64(30)}, ty, bl)) == WIT_OUT_OF_RANGE, "the output at hi");
  CHECK(status(st, typed(132, 100, 30)) == WIT_UNBALANCED, "an unbalanced witness");
  CHECK(status(st, typed(131, -21, 30)) == WIT_UNBALANCED, "out of range and unbalanced: the balance comes first");
  CHECK(status(st, typed(131, 100, 700)) == WIT_UNBALANCED && status(st, typed(801, 100, 700)) == WIT_OK, "the assumed range is not checked");
  { Row r = typed(131, 100, 30); N.store(&r.bld[4]); CHECK(status(st, r) == WIT_NOT_CANONICAL, "a blinding of n"); }
  { Row r = typed(132, -21, 30); u_add(N, t15).store(&r.typ[8]); CHECK(status(st, r) == WIT_NOT_CANONICAL, "canonical comes before balance and range"); }
  { const U256 fee = U256::from_u64(5); CHECK(status(st, typed(135, 100, 30), &fee) == WIT_OK && status(st, typed(131, 100, 30), &fee) == WIT_UNBALANCED, "a public amount per proof"); }
  { Row r = row({U256::from_u64(131), U256::from_u64(100), U256::from_u64(30)}, {t15, U256::from_u64(16), t15}, bl);
    CHECK(status(st, r) == WIT_UNBALANCED, "types balance one by one"); }
  // an untyped setup has no balance
  { Setup su; CHECK(make_setup(false, rds, {}, su, err, 0), "untyped: %s", err.c_str());
    CHECK(status(su, typed(5, 6, 7)) == WIT_OK && status(su, typed(-1, 6, 7)) == WIT_OUT_OF_RANGE, "untyped"); }
  // ---- bin_test
  std::vector<RangeData> brds(3);
  CHECK(make_range_data_binary(U256::from_u64(3), pow2(64), true, false, brds[0], err), "binary range 0");
  CHECK(make_range_data_binary(U256::from_u64(2), pow2(64), false, true, brds[1], err) && make_range_data_binary(U256::from_u64(2), pow2(64), false, true, brds[2], err), "binary inputs");
  Setup sb;
  CHECK(make_setup_binary(true, brds, U256::from_u64(2), 0, sb, err), "bin_test: %s", err.c_str());
  auto bin = [&](long long out, long long in1, long long in2) { return row({from_i64(out), from_i64(in1), from_i64(in2)}, ty, bl); };
  CHECK(status(sb, bin(102, 60, 40)) == WIT_OK, "a balanced binary witness refused");
  CHECK(status(sb, bin(2, 0, 0)) == WIT_OUT_OF_RANGE, "the output below 3");
  CHECK(status(sb, bin(103, 60, 40)) == WIT_BIN_UNBALANCED, "an unbalanced binary witness");
  { Row r = bin(102, 60, 40); N.store(&r.bld[8]); CHECK(status(sb, r) == WIT_BIN_NOT_CANONICAL, "a binary blinding of n"); }
  { Row r = bin(2, 0, 0); N.store(&r.bld[8]); CHECK(status(sb, r) == WIT_OUT_OF_RANGE, "range 0's bounds come before range 2's blinding"); }
  { Row r = bin(2, 0, 0); N.store(&r.bld[0]); CHECK(status(sb, r) == WIT_BIN_NOT_CANONICAL, "a range's blinding comes before its bounds"); }
  { const U256 net = U256::from_u64(7); CHECK(status(sb, bin(107, 60, 40), &net) == WIT_OK && status(sb, bin(102, 60, 40), &net) == WIT_BIN_UNBALANCED, "a net amount per proof"); }
  { Setup s0; CHECK(make_setup_binary(false, brds, U256::zero(), 0, s0, err), "no conservation");
    CHECK(status(s0, bin(100, 60, 40)) == WIT_BIN_UNBALANCED, "a binary witness needs a conserved schema (Binary.hs:162-164)"); }
  for (uint32_t s = 1; s <= 5; s++) CHECK(std::string(wit_status_text(s)) != wit_status_text(0), "status %u has no text", s);
  printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
