// CPU build of fp30.cuh's ATOM-WISE Montgomery product (f30_prod::step, f30_run1, f30_run2 and the generated schedules of
// mac30_asm.cuh), for tests/test_fp30_atoms_host.py only: KZG_FP30_HOST_ATOMS makes the CPU build take the code the device
// runs, with the C fallback of every generated statement, next to the column-wise f30_mul_core_c it must agree with.
#include <stdint.h>
#include <string.h>

#define KZG_FP30_HOST_ATOMS 1
#include "../../kateth_amd/csrc/fp30.cuh"

using namespace kzg;

// ops[6][13]: a, b, c, d, inj0, inj1
static void load6(fp30* o, const int32_t* ops) {
  for (int k = 0; k < 6; k++) memcpy(o[k].l, ops + 13 * k, sizeof(o[k].l));
}

template <bool SQR, bool TWO, int C0, int C1, bool U>
static void one(int atoms, int32_t* out, const int32_t* ops) {
  fp30 o[6], r;
  load6(o, ops);
  if (atoms)
    f30_mul_core<SQR, TWO, C0, C1, U>(r, o[0], o[1], o[2], o[3], o[4], o[5]);
  else
    f30_mul_core_c<SQR, TWO, C0, C1, U>(r, o[0], o[1], o[2], o[3], o[4], o[5]);
  memcpy(out, r.l, sizeof(r.l));
}

// variant: 0 product, 1 squaring, 2 double product, 3 product with -1 injected, 4 squaring with -1, -3 injected, 5 U-form product
extern "C" int hma_one(int variant, int atoms, int32_t* out13, const int32_t* ops) {
  switch (variant) {
    case 0: one<false, false, 0, 0, false>(atoms, out13, ops); return 0;
    case 1: one<true, false, 0, 0, false>(atoms, out13, ops); return 0;
    case 2: one<false, true, 0, 0, false>(atoms, out13, ops); return 0;
    case 3: one<false, false, -1, 0, false>(atoms, out13, ops); return 0;
    case 4: one<true, false, -1, -3, false>(atoms, out13, ops); return 0;
    case 5: one<false, false, 0, 0, true>(atoms, out13, ops); return 0;
  }
  return 1;
}

template <bool SA, bool TA, int C0A, int C1A, bool UA, bool SB, bool TB, int C0B, int C1B, bool UB>
static void two(int atoms, int32_t* outa, int32_t* outb, const int32_t* opsa, const int32_t* opsb) {
  fp30 x[6], y[6], ra, rb;
  load6(x, opsa);
  load6(y, opsb);
  if (atoms) {
    f30_mul_core2<SA, TA, C0A, C1A, UA, SB, TB, C0B, C1B, UB>(ra, x[0], x[1], x[2], x[3], x[4], x[5], rb, y[0], y[1], y[2], y[3], y[4], y[5]);
  } else {
    f30_mul_core_c<SA, TA, C0A, C1A, UA>(ra, x[0], x[1], x[2], x[3], x[4], x[5]);
    f30_mul_core_c<SB, TB, C0B, C1B, UB>(rb, y[0], y[1], y[2], y[3], y[4], y[5]);
  }
  memcpy(outa, ra.l, sizeof(ra.l));
  memcpy(outb, rb.l, sizeof(rb.l));
}

// the four pairs of xyzz30_madd_fast, in its order: PP with R, PPP with Q, V with ZZ3, -Y3 with ZZZ3
extern "C" int hma_pair(int pair, int atoms, int32_t* outa, int32_t* outb, const int32_t* opsa, const int32_t* opsb) {
  switch (pair) {
    case 0: two<true, false, 0, 0, false, false, false, -1, 0, false>(atoms, outa, outb, opsa, opsb); return 0;
    case 1: two<false, false, 0, 0, false, false, false, 0, 0, false>(atoms, outa, outb, opsa, opsb); return 0;
    case 2: two<true, false, -1, -3, false, false, false, 0, 0, true>(atoms, outa, outb, opsa, opsb); return 0;
    case 3: two<false, true, 0, 0, false, false, false, 0, 0, true>(atoms, outa, outb, opsa, opsb); return 0;
  }
  return 1;
}
