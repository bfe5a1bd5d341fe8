/* Prints the layout of every public struct of include/iqdemod_fsk.h as the C compiler sees it, in abi_layout_check.c's
 * format: one line "struct <name> <sizeof>", then one line "<name>.<field> <offsetof> <size>" per field, in the header's
 * order.  tests/test_fsk_host.py holds the lines against the header's own field lists and against the mirrors of
 * rtlsdrdiags_amd/fsk.py.  Plain C99, no library. */
#include <stddef.h>
#include <stdio.h>

#include "iqdemod_fsk.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("%s.%s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T *)0)->f))

int main(void)
{
    S(iqd_fsk_config);
    F(iqd_fsk_config, abi_version); F(iqd_fsk_config, n_channels); F(iqd_fsk_config, corr_len); F(iqd_fsk_config, mark_inc);
    F(iqd_fsk_config, space_inc); F(iqd_fsk_config, baud_inc); F(iqd_fsk_config, loop_shift); F(iqd_fsk_config, flags);
    F(iqd_fsk_config, window); F(iqd_fsk_config, min_len); F(iqd_fsk_config, max_len); F(iqd_fsk_config, reserved);

    S(iqd_fsk_frame);
    F(iqd_fsk_frame, end_sample); F(iqd_fsk_frame, offset); F(iqd_fsk_frame, len); F(iqd_fsk_frame, fcs); F(iqd_fsk_frame, flags);

    S(iqd_fsk_state);
    F(iqd_fsk_state, samples); F(iqd_fsk_state, ph); F(iqd_fsk_state, prev); F(iqd_fsk_state, last); F(iqd_fsk_state, ones);
    F(iqd_fsk_state, in_frame); F(iqd_fsk_state, nbits); F(iqd_fsk_state, bad_fcs); F(iqd_fsk_state, frames_total);
    return 0;
}
