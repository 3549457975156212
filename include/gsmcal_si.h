/* gsmcal_si.h -- the small message parser behind gsmcal_BCCH_decode: what a decoded BCCH block says about
 * the cell.  Plain C99, header only, nothing of HIP or of the library in it: it can be compiled into any program on its own.
 *
 * A block is 23 octets.  Octet 0 is the L2 pseudo-length, (length << 2) | 1; octet 1 the protocol discriminator 0x06 (radio
 * resources, skip indicator 0); octet 2 the message type: 0x19 / 0x1A / 0x1B / 0x1C for SYSTEM INFORMATION TYPE 1 / 2 / 3 / 4
 * (GSM 04.08 section 10.4).  Type 3 carries the cell identity in octets 3-4 (big-endian) and the location area identification in
 * octets 5-9; type 4 the location area identification in octets 3-7.  The location area identification (04.08 section 10.5.1.3):
 * MCC digit 2 | MCC digit 1, MNC digit 3 | MCC digit 3, MNC digit 2 | MNC digit 1 (BCD, high nibble first named), then the LAC
 * big-endian; a 2-digit MNC has the filler 0xF as its third digit.  The rest octets and every other field are not looked at.
 * The octet and bit order of the block is unpinned against a real capture; synth.si_fields is the same
 * parser in Python. */
#ifndef GSMCAL_SI_H
#define GSMCAL_SI_H

#ifdef __cplusplus
extern "C" {
#endif

#define GSMCAL_SI_OCTETS 23

typedef struct gsmcal_si_info {
    int valid;      /* 1: a recognised message whose fields below are filled in; 0: anything else                       */
    int msg_type;   /* octet 2 as it is                                                                                  */
    int si_type;    /* 1..4 for SYSTEM INFORMATION TYPE 1..4, 0 otherwise                                                */
    int cell_id;    /* type 3: 0..65535; -1 otherwise                                                                    */
    int mcc;        /* types 3 and 4: 0..999; -1 otherwise                                                               */
    int mnc;        /* types 3 and 4: 0..99 (2 digits) or 0..999 (3 digits); -1 otherwise                                */
    int mnc_digits; /* 2 or 3; -1 otherwise                                                                              */
    int lac;        /* types 3 and 4: 0..65535; -1 otherwise                                                             */
} gsmcal_si_info;

/* The function is `static inline` for a program that includes this header; libgsmcal.so defines GSMCAL_SI_LINKAGE empty and so
 * exports the one definition under the same name (the ctypes mirror calls that one). */
#ifndef GSMCAL_SI_LINKAGE
#define GSMCAL_SI_LINKAGE static inline
#endif

/* Returns info->valid.  valid = 0 for anything the parser does not recognise: a pseudo-length octet whose low two bits are not
 * 01, another protocol discriminator, another message type, a BCD digit above 9 other than the filler in the MNC's third place. */
GSMCAL_SI_LINKAGE int gsmcal_si_fields(const unsigned char octets[GSMCAL_SI_OCTETS], gsmcal_si_info* info) {
    int at, m[3], n[3];
    if (!info) return 0;
    info->valid = 0;
    info->msg_type = octets ? octets[2] : -1;
    info->si_type = 0;
    info->cell_id = info->mcc = info->mnc = info->mnc_digits = info->lac = -1;
    if (!octets || (octets[0] & 3) != 1 || octets[1] != 0x06) return 0;
    if (octets[2] < 0x19 || octets[2] > 0x1C) return 0;
    info->si_type = octets[2] - 0x18;
    if (info->si_type < 3) return (info->valid = 1);
    at = info->si_type == 3 ? 5 : 3;
    m[0] = octets[at] & 15;
    m[1] = octets[at] >> 4;
    m[2] = octets[at + 1] & 15;
    n[0] = octets[at + 2] & 15;
    n[1] = octets[at + 2] >> 4;
    n[2] = octets[at + 1] >> 4;
    if (m[0] > 9 || m[1] > 9 || m[2] > 9 || n[0] > 9 || n[1] > 9 || (n[2] > 9 && n[2] != 15)) return 0;
    if (info->si_type == 3) info->cell_id = (octets[3] << 8) | octets[4];
    info->mcc = 100 * m[0] + 10 * m[1] + m[2];
    info->mnc_digits = n[2] == 15 ? 2 : 3;
    info->mnc = n[2] == 15 ? 10 * n[0] + n[1] : 100 * n[0] + 10 * n[1] + n[2];
    info->lac = (octets[at + 3] << 8) | octets[at + 4];
    return (info->valid = 1);
}

#ifdef __cplusplus
}
#endif
#endif
