"""LDS bank-conflict enumeration for wgrad_bf16_kernel (csrc/wgrad.hip): for candidate row strides LDT (16-bit elements) and chunk swizzles s(row),
the worst conflict degree of the ds_read_b128 fragment reads (16-lane service groups, 64 banks of 16-B slots) and of the transposing
ds_write_b32 of the X tile (32-lane groups, 32 banks), per MI355X_MICROARCH.md section LDS.  Round 1-5 layout = (72, none): reads 1, writes 16."""
import itertools
G128=[[0,1,2,3,12,13,14,15,20,21,22,23,24,25,26,27],[4,5,6,7,8,9,10,11,16,17,18,19,28,29,30,31]]
G128=G128+[[l+32 for l in g] for g in G128]
def read_conf(LDT, s):
    # ds_read_b128: lane -> row = wave*32 + (lane&31), chunk = kk*2 + (lane>>5); bank64 of 16-B slot
    worst=0
    for wave in range(4):
        for kk in range(4):
            for g in G128:
                slots={}
                for l in g:
                    row=wave*32+(l&31); ch=(kk*2+(l>>5))^s(row)
                    a=row*LDT*2+ch*16
                    slot=(a//16)%16
                    slots.setdefault(slot,set()).add(a)
                worst=max(worst,max(len(v) for v in slots.values()))
    return worst
def write_conf_x(LDT, s):
    # ds_write_b32, 2 groups of 32 lanes; thread tid: xc=tid&15, xp0=tid>>4; h in 0,1; i in 0..7
    worst=0
    for wave in range(4):
        for half in range(2):
            for h in range(2):
                for i in range(8):
                    banks={}
                    for l in range(32):
                        tid=wave*64+half*32+l
                        xc=tid&15; xp0=tid>>4
                        row=xc*8+i; tok=2*(xp0+16*h)
                        ch=(tok//8)^s(row)
                        a=row*LDT*2+ch*16+(tok%8)*2
                        b=(a//4)%32
                        banks.setdefault(b,set()).add(a)
                    worst=max(worst,max(len(v) for v in banks.values()))
    return worst
cands={}
for LDT in (64,72,80):
    for name,s in {
        "none":lambda r:0,
        "r>>3":lambda r:(r>>3)&7,
        "r&7":lambda r:r&7,
        "(r>>3)^(r&7)":lambda r:((r>>3)^r)&7,
        "(r>>1)&7":lambda r:(r>>1)&7,
        "(r>>2)&7":lambda r:(r>>2)&7,
        "(r>>3)+(r>>6)":lambda r:((r>>3)+(r>>6))&7,
        "((r>>3)&7)^((r>>2)&1)":lambda r:((r>>3)&7)^((r>>2)&1),
        "(r>>3 ^ r>>1)&7":lambda r:((r>>3)^(r>>1))&7,
        "(r>>3 ^ r<<1)&7":lambda r:((r>>3)^(r<<1))&7,
        "(r>>3 ^ r<<2)&7":lambda r:((r>>3)^(r<<2))&7,
    }.items():
        print(LDT,name,"read",read_conf(LDT,s),"writeX",write_conf_x(LDT,s))
