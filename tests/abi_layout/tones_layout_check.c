/* Prints the layout of every public struct of include/iqdemod_tones.h as the C compiler sees it, in abi_layout_check.c's
 * format: one line "struct <name> <sizeof>", then one line "<name>.<field> <offsetof> <size>" per field, in the header's
 * order.  tests/test_tones_host.py holds the lines against the header's own field lists and against the mirrors of
 * rtlsdrdiags_amd/tones.py.  Plain C99, no library. */
#include <stddef.h>
#include <stdio.h>

#include "iqdemod_tones.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("%s.%s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T *)0)->f))

int main(void)
{
    S(iqd_tones_config);
    F(iqd_tones_config, abi_version); F(iqd_tones_config, n_channels); F(iqd_tones_config, frame_len); F(iqd_tones_config, n_tones);
    F(iqd_tones_config, phase_inc); F(iqd_tones_config, window); F(iqd_tones_config, min_power); F(iqd_tones_config, ratio_q8);
    F(iqd_tones_config, energy_q8); F(iqd_tones_config, open); F(iqd_tones_config, hold); F(iqd_tones_config, reserved);

    S(iqd_tones_frame);
    F(iqd_tones_frame, energy); F(iqd_tones_frame, p_best); F(iqd_tones_frame, p_second); F(iqd_tones_frame, best);
    F(iqd_tones_frame, second); F(iqd_tones_frame, tone); F(iqd_tones_frame, flags);

    S(iqd_tones_state);
    F(iqd_tones_state, tone); F(iqd_tones_state, cand); F(iqd_tones_state, run); F(iqd_tones_state, miss); F(iqd_tones_state, fill);
    F(iqd_tones_state, reserved);
    return 0;
}
