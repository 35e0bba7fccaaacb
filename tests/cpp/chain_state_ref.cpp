// bl_serial_sum.h's own definitions, array by array, for tests/test_chain_state_model.py (built as a shared object by the test):
// ss_from (the ldexpf form), ss_acc_float (the bit-pattern form the chain uses), ss_rec_fits.
#include "../../botlab_amd/csrc/bl_serial_sum.h"

extern "C" {

// out[i] = bits of ss_from(key[i], M[i])
void csr_from(const int* key, const int* M, uint32_t* out, int n)
{
    for (int i = 0; i < n; ++i) out[i] = ss_f2u(ss_from(key[i], M[i]));
}

// out[i] = bits of ss_acc_float({key[i], M[i]})
void csr_acc_float(const int* key, const int* M, uint32_t* out, int n)
{
    for (int i = 0; i < n; ++i) { ss_acc a; a.key = key[i]; a.M = M[i]; out[i] = ss_f2u(ss_acc_float(a)); }
}

// key_out[i], M_out[i] = ss_acc_of(the float with bits[i])
void csr_acc_of(const uint32_t* bits, int* key_out, int* M_out, int n)
{
    for (int i = 0; i < n; ++i) { const ss_acc a = ss_acc_of(ss_u2f(bits[i])); key_out[i] = a.key; M_out[i] = a.M; }
}

// rec[4 i ..]: key, D, lo, hi.  fits[i] = ss_rec_fits; out[i] = bits of ss_from(key[i], M[i] + D) where it fits, else 0
void csr_gap(const int* rec, const int* key, const int* M, int* fits, uint32_t* out, int n)
{
    for (int i = 0; i < n; ++i) {
        const ss_rec r = ss_rec_make(rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]);
        fits[i] = ss_rec_fits(r, key[i], M[i]) ? 1 : 0;
        out[i] = fits[i] ? ss_f2u(ss_from(key[i], M[i] + r.D)) : 0u;
    }
}

}
